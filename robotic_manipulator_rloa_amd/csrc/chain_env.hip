// Kinematic environment of a user's manipulator, E independent copies stepped on the device: the serial chain that
// environment/urdf_chain.py compiles from a URDF (driven joints with folded pre-transforms, capsule segments, observation
// slots), under the reference's environment rule — the contract csrc/synth_env.hip keeps for its one hard-wired chain:
//   state  = [pos(A), vel(A), end-effector xyz, target xyz, obstacle xyz]   (environment.py:431-451, S = 9+2A; slot k of
//            pos / vel reports joint INDEX k, environment.py:442-444)
//   reward = +250 on reaching the target (dist < 0.05), -1000 on obstacle contact, else -(dist - 0.05)
//            (environment.py:345-371, :419-429);  done = 1 on either (environment.py:311-333)
//   step   = velocity control for one 1/240 s tick, applied exactly, then the position limits (environment.py:453-485)
// NOT a port of Bullet: no dynamics, no mesh collision. Self-collision is the reference's rule (environment.py:311-343, :394-412;
// collision_detector.py:63-98) between capsules, for the segment pairs the blob lists. environment/kinematic.py is its float64 twin.
//
// One lane per env, 64-lane workgroups. The model is the same for every lane and is read through a uniform pointer with
// uniform indices (scalar loads / one broadcast line); nothing of it is copied into per-lane arrays. The walk keeps only the
// current frame (R, p) in registers; joint values and actions are read from and written to env_state / the row as the walk
// reaches them, so there is no runtime-indexed per-lane array and nothing goes to scratch, at any A <= 64.
//
// Self-collision (P > 0 pairs in the blob) is a second instantiation of the same kernels, SC = true; with P = 0 the launch is
// the SC = false one: no LDS, one wave per workgroup, the rows it always wrote. With SC the walking wave also stores each
// capsule's two world end points in LDS as [segment][6][lane] floats — lane-contiguous, so every access is one conflict-free
// row and no per-lane array is indexed at run time — and the workgroup has W waves: wave 0 walks, a barrier, then pair p is
// tested by wave p mod W (lane = env, pair indices and radii through uniform loads), each wave leaves the minimum of its pairs'
// clearances in LDS, a barrier, and wave 0 takes the minimum of the W before it writes reward and done.
//
// Scene ranges (naf_chain_env_set_scene_ranges, a non-zero half-width) are a further instantiation of the reset and step kernels,
// SCENE = true; with all half-widths zero the launch is the SCENE = false one. Every episode then starts with a scene of its
// own: after the joint draw the CH_TRIES obstacle candidates are drawn, the ONE walk of the reset pose collects each
// candidate's clearance beside the end effector (CH_TRIES clearances in registers, every loop over them unrolled), and the first
// candidate that meets the three conditions of include/naf_hip.h becomes the scene, the nominal scene if none does. No trip count
// depends on a draw. In an SC workgroup this is the walking wave's business alone, as the auto-reset already is.
//
// Workcell (G + H > 0 fixed spheres and half-spaces in the blob) is one more instantiation of the step and rollout kernels,
// CELL = true, and a probe of its own; without one the launches are the CELL-less kernels, unchanged. The walk tests each capsule,
// behind its obstacle test, against the geometries its mask names: counts, mask and geometry come through uniform loads, the
// trip counts are uniform, and nothing is kept per lane but the running minimum. The walk of an auto-reset pose does not test.
//
// Boxes (B > 0 rounded oriented boxes in the blob) are one more instantiation again, BOX = true, of the CELL kernels and of the
// probe: behind the sphere and half-space loop the capsule's segment is taken into each box's frame and its distance to the box is
// found in closed form (seg_box_dist2: eight knots, a fixed trip count, the running bracket of the derivative the only state).
// The BOX kernels test the model's spheres and half-spaces too; a model without a box launches the kernels it always did.
#include "common.h"
#include "../../include/naf_hip.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <new>
#include <type_traits>
#include <vector>

#define CH_DT (1.0f / 240.0f)
#define CH_MAX_A NAF_MAX_A_WIDE
// blob offsets (include/naf_hip.h, "chain model blob")
#define CH_HDR NAF_CHAIN_HEADER_FLOATS
#define CH_JNT NAF_CHAIN_JOINT_FLOATS
#define CH_SEG NAF_CHAIN_SEGMENT_FLOATS
#define CH_TRIES NAF_CHAIN_SCENE_TRIES
#define CH_BOX NAF_CHAIN_BOX_FLOATS
#define CH_REACHED 0.05f                     // the target threshold of the reward rule

struct naf_chain_env {
    float* model_dev;
    int n_floats, A, n_seg;
    int n_cell;                     // G + H + B: workcell geometries in the blob (0: the CELL-less kernels are launched)
    int n_box;                      // B of them boxes (0: the launches are the ones of a model without boxes)
    int n_pairs, lanes, waves;      // P; with P > 0: envs per workgroup (64, 32, .. 1) and waves per workgroup
    float ranges[NAF_CHAIN_RANGE_FLOATS];      // set_scene_ranges: target half-widths | obstacle half-widths | margin
    float centre[6];                // target | obstacle of the last reset's scene_host: the boxes' centres and the fallback
    bool scene_on, scene_ready;     // a half-width is non-zero; a reset has run since the ranges were set
    int ee_frame;                  // the end-effector frame: the goal-pose solver walks the joints before it
};
#ifndef CH_MAX_WAVES
#define CH_MAX_WAVES 16                      // (-DCH_MAX_WAVES=1 through NAF_BUILD_DEFINES: the one-wave pair loop, NOTEBOOK §15)
#endif
// A SCENE launch holds CH_TRIES candidates and clearances through the walk of a reset pose: its workgroups are at most 8 waves
// (SC; the pair phase takes any wave count and its minimum does not depend on it) or one (no SC), so that the register
// budget, which the launch bound sets, holds them without scratch.
#define CH_SCENE_WAVES (CH_MAX_WAVES < 8 ? CH_MAX_WAVES : 8)
#define CH_PAIRS_PER_WAVE 16                 // waves = ceil(P / this), at most CH_MAX_WAVES
#define CH_MAX_DYN_LDS (144 * 1024)          // of the CU's 160 KiB; the SC kernels have no static LDS beside it
#define CH_WG_LDS (160 * 1024)               // all a gfx950 workgroup may take: the cap of an entry that adds tables behind the rows

struct ChainScene {
    float v[NAF_CHAIN_SCENE_FLOATS];    // target | obstacle | jitter | obstacle radius
};

// what a SCENE launch draws from: target | obstacle centres, target | obstacle half-widths, margin
struct ChainRanges {
    float centre[6], half[6], margin;
};
// the obstacle candidates of one reset and, after the walk, each one's min over the capsules of (distance - capsule radius)
struct SceneCand {
    float o[CH_TRIES][3], clear[CH_TRIES];
};
// The kernels take the ranges as a trailing parameter PACK: one ChainRanges in a SCENE launch, nothing in a SCENE = false one,
// whose kernel arguments are then exactly those of the kernels before the ranges existed.
// a further, empty member of the pack: the launch tests the workcell (chain_env_step_kernel)
struct ChainCell {};
// and one more, last in the pack: the row's last float carries the 1-based ordinal of the env's current episode (hindsight
// relabelling in the replay gather asks for it; 0, what every launch without it leaves there, means "untagged")
struct ChainTag {};
// a third empty member, behind ChainCell: the model holds boxes, which the walk tests behind the spheres and half-spaces
struct ChainBox {};
template <class... Rest>
__device__ static inline const ChainRanges& scene_ranges(const ChainRanges& rg, const Rest&...) { return rg; }

__host__ __device__ static inline int ch_off_begin(int A) { return CH_HDR + CH_JNT * A; }
__host__ __device__ static inline int ch_off_seg(int A) { return ch_off_begin(A) + A + 2; }
__host__ __device__ static inline int ch_off_slot(int A, int n_seg) { return ch_off_seg(A) + CH_SEG * n_seg; }
__host__ __device__ static inline int ch_off_pair(int A, int n_seg) { return ch_off_slot(A, n_seg) + 2 * A; }
// the workcell section: G spheres, H half-spaces (4 floats each), B boxes (CH_BOX floats each), then n_seg masks
__host__ __device__ static inline int ch_off_cell(int A, int n_seg, int n_pairs) { return ch_off_pair(A, n_seg) + 2 * n_pairs; }
// dynamic LDS of an SC launch: end points [n_seg][6][lanes], then one minimum per (wave, lane)
__host__ __device__ static inline size_t ch_lds_bytes(int n_seg, int lanes, int waves) {
    return ((size_t)n_seg * 6 + waves) * lanes * sizeof(float);
}
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

// squared distance between the segments a-b and c-d. The minimum over five candidates, each between two points that lie on the
// two segments (so none is below the answer): the carrying lines' closest points — closed form with a guarded denominator,
// clamped, then each parameter projected once more given the other — and the four end-point-to-segment distances. The minimum
// over the parameter square is interior (the lines' pair) or has a parameter at 0 or 1 (an end point against the other
// segment); parallel and zero-length segments, where the denominator vanishes, attain theirs at an end point.
__device__ static inline float seg_seg_dist2(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                             float dx, float dy, float dz) {
    const float ux = bx - ax, uy = by - ay, uz = bz - az;
    const float vx = dx - cx, vy = dy - cy, vz = dz - cz;
    const float wx = ax - cx, wy = ay - cy, wz = az - cz;
    const float a = ux * ux + uy * uy + uz * uz, b = ux * vx + uy * vy + uz * vz, c = vx * vx + vy * vy + vz * vz;
    const float d = ux * wx + uy * wy + uz * wz, e = vx * wx + vy * wy + vz * wz;
    const float den = a * c - b * b;
    float s = den > 1e-7f * a * c ? (b * e - c * d) / den : 0.f;
    s = fminf(1.f, fmaxf(0.f, s));
    float t = c > 0.f ? (b * s + e) / c : 0.f;
    t = fminf(1.f, fmaxf(0.f, t));
    s = a > 0.f ? (b * t - d) / a : 0.f;
    s = fminf(1.f, fmaxf(0.f, s));
    const float xx = wx + s * ux - t * vx, xy = wy + s * uy - t * vy, xz = wz + s * uz - t * vz;
    float best = xx * xx + xy * xy + xz * xz;
    best = fminf(best, seg_point_dist2(cx, cy, cz, dx, dy, dz, ax, ay, az));
    best = fminf(best, seg_point_dist2(cx, cy, cz, dx, dy, dz, bx, by, bz));
    best = fminf(best, seg_point_dist2(ax, ay, az, bx, by, bz, cx, cy, cz));
    best = fminf(best, seg_point_dist2(ax, ay, az, bx, by, bz, dx, dy, dz));
    return best;
}

// half of f'(t) for f(t) = sum_i max(|p_i + t u_i| - h_i, 0)^2: sum_i (x_i - clamp(x_i, -h_i, h_i)) u_i at x = p + t u
__device__ static inline float box_slope(float t, float px, float py, float pz, float ux, float uy, float uz, float hx, float hy,
                                         float hz) {
    const float x = fmaf(t, ux, px), y = fmaf(t, uy, py), z = fmaf(t, uz, pz);
    return (x - fminf(hx, fmaxf(-hx, x))) * ux + (y - fminf(hy, fmaxf(-hy, y))) * uy + (z - fminf(hz, fmaxf(-hz, z))) * uz;
}

// squared distance from the segment p + t u, t in [0, 1], to the box |x_i| <= h_i, all in the box's frame. f is convex and
// piecewise quadratic, so f' is non-decreasing and linear between its knots: 0, 1 and the six (+-h_i - p_i) / u_i clipped into
// [0, 1] (an axis with u_i = 0 has none: its two fall on the knot 0). The largest knot with f' <= 0 and the smallest with f' >= 0
// bracket the minimum, which is where the line through them crosses 0; f' > 0 at 0 puts it at 0, f' < 0 at 1 at 1. No sort, no
// iteration, and only the bracket is live across the knots.
__device__ static inline float seg_box_dist2(float px, float py, float pz, float ux, float uy, float uz, float hx, float hy,
                                             float hz) {
    float t_lo = 0.f, t_hi = 1.f;
    float g_lo = box_slope(0.f, px, py, pz, ux, uy, uz, hx, hy, hz), g_hi = box_slope(1.f, px, py, pz, ux, uy, uz, hx, hy, hz);
    const float g0 = g_lo, g1 = g_hi;
    const float p[3] = {px, py, pz}, u[3] = {ux, uy, uz}, h[3] = {hx, hy, hz};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int i = k >> 1;
        const float inv = u[i] != 0.f ? 1.f / u[i] : 0.f;
        const float t = fminf(1.f, fmaxf(0.f, ((k & 1 ? h[i] : -h[i]) - p[i]) * inv));
        const float g = box_slope(t, px, py, pz, ux, uy, uz, hx, hy, hz);
        const bool lo = g <= 0.f && t >= t_lo, hi = g >= 0.f && t <= t_hi;
        t_lo = lo ? t : t_lo;
        g_lo = lo ? g : g_lo;
        t_hi = hi ? t : t_hi;
        g_hi = hi ? g : g_hi;
    }
    const float den = g_hi - g_lo;
    float t = den > 0.f ? t_lo - g_lo * (t_hi - t_lo) / den : t_lo;
    t = fminf(t_hi, fmaxf(t_lo, t));
    t = g0 > 0.f ? 0.f : (g1 < 0.f ? 1.f : t);
    const float x = fmaf(t, ux, px), y = fmaf(t, uy, py), z = fmaf(t, uz, pz);
    const float ex = fmaxf(fabsf(x) - hx, 0.f), ey = fmaxf(fabsf(y) - hy, 0.f), ez = fmaxf(fabsf(z) - hz, 0.f);
    return ex * ex + ey * ey + ez * ez;
}

// Where the SC instantiations keep the capsules' world end points: `ends` is the LDS array already offset by the lane, `lanes`
// its innermost extent. CLEAR: `clear` collects min over the capsules of (distance to the obstacle centre - capsule radius),
// and with CELL `cell` the workcell clearance: min over the tested (capsule, geometry) pairs.
// CERT (the certifying path kernel): `beta` is the lane's table of half-steps, one entry per segment, and `slack` / `cell_slack`
// collect the same two minima with the segment's entry subtracted from every test.
struct WalkAux {
    float* ends;
    int lanes;
    float clear;
    float cell;
    const float* beta;
    float slack;
    float cell_slack;
};

// contact of the capsules of frame f with the obstacle sphere, and the end-effector point when it lives in f. CELL: also their
// contact with the workcell — ORed into the result, except with CLEAR, where aux.cell < 0 says it and the result stays the
// obstacle's own (the rollout tells the two apart).
template <bool SC, bool PROBE, bool SCENE = false, bool CLEAR = PROBE, bool CELL = false, bool BOX = false, bool CERT = false>
__device__ static inline bool frame_geometry(const float* __restrict__ model, int A, int f, const Frame& F, float ox, float oy,
                                             float oz, float orad, int ee_frame, float* ee, WalkAux& aux, SceneCand* cand = nullptr) {
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
        const float d2 = seg_point_dist2(ax, ay, az, bx, by, bz, ox, oy, oz);
        hit |= d2 < rr * rr;
        if constexpr (SC) {
            float* w = aux.ends + (size_t)s * 6 * aux.lanes;
            w[0] = ax; w[aux.lanes] = ay; w[2 * aux.lanes] = az;
            w[3 * aux.lanes] = bx; w[4 * aux.lanes] = by; w[5 * aux.lanes] = bz;
        }
        if constexpr (CLEAR) aux.clear = fminf(aux.clear, sqrtf(d2) - g[7]);
        if constexpr (CERT) aux.slack = fminf(aux.slack, sqrtf(d2) - g[7] - aux.beta[s]);
        if constexpr (CELL) {
            const int n_sph = (int)model[10], n_geo = n_sph + (int)model[11];
            const float* geo = model + ch_off_cell(A, (int)model[2], (int)model[9]);
            int mask;
            if constexpr (BOX) mask = (int)geo[4 * n_geo + CH_BOX * (int)model[12] + s];
            else mask = (int)geo[4 * n_geo + s];
            float least = INFINITY;
            for (int k = 0; k < n_geo; ++k) {      // (uniform: the counts, the mask and the geometry are the blob's)
                if (!(mask >> k & 1)) continue;
                const float* c = geo + 4 * k;
                float d;
                if (k < n_sph) {
                    d = sqrtf(seg_point_dist2(ax, ay, az, bx, by, bz, c[0], c[1], c[2])) - c[3];
                } else {
                    const float na = c[0] * ax + c[1] * ay + c[2] * az, nb = c[0] * bx + c[1] * by + c[2] * bz;
                    d = fminf(na, nb) - c[3];
                }
                least = fminf(least, d - g[7]);
            }
            if constexpr (BOX) {
                // the boxes' records lie between the G + H records and the masks; geometry index n_geo + k
                const int n_box = (int)model[12], bmask = mask >> n_geo;
                const float wx = bx - ax, wy = by - ay, wz = bz - az;
                for (int k = 0; k < n_box; ++k) {      // (uniform, as above)
                    if (!(bmask >> k & 1)) continue;
                    const float* x = geo + 4 * n_geo + CH_BOX * k;      // c | R row-major | h | r
                    const float ex = ax - x[0], ey = ay - x[1], ez = az - x[2];
                    const float d2 = seg_box_dist2(x[3] * ex + x[6] * ey + x[9] * ez, x[4] * ex + x[7] * ey + x[10] * ez,
                                                   x[5] * ex + x[8] * ey + x[11] * ez, x[3] * wx + x[6] * wy + x[9] * wz,
                                                   x[4] * wx + x[7] * wy + x[10] * wz, x[5] * wx + x[8] * wy + x[11] * wz, x[12],
                                                   x[13], x[14]);
                    least = fminf(least, sqrtf(d2) - x[15] - g[7]);
                }
            }
            if constexpr (CLEAR) aux.cell = fminf(aux.cell, least);
            else hit |= least < 0.f;
            // (the entry is the segment's, the same for every geometry: one subtraction behind the minimum over them)
            if constexpr (CERT) aux.cell_slack = fminf(aux.cell_slack, least - aux.beta[s]);
        }
        if constexpr (SCENE) {
            // seg_point_dist2 for CH_TRIES centres against ONE segment: its direction and 1 / |u|^2 are computed once, and the
            // root is the hardware's (1 ulp): both far inside the band in which the choice is compared with the twin's
            const float ux = bx - ax, uy = by - ay, uz = bz - az;
            const float den = ux * ux + uy * uy + uz * uz;
            const float inv = den > 0.f ? 1.f / den : 0.f;
#pragma unroll
            for (int c = 0; c < CH_TRIES; ++c) {
                const float wx = cand->o[c][0] - ax, wy = cand->o[c][1] - ay, wz = cand->o[c][2] - az;
                const float t = fminf(1.f, fmaxf(0.f, (wx * ux + wy * uy + wz * uz) * inv));
                const float dx = wx - t * ux, dy = wy - t * uy, dz = wz - t * uz;
                cand->clear[c] = fminf(cand->clear[c], __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz) - g[7]);
            }
        }
    }
    if (f == ee_frame) {
        ee[0] = F.px + F.r00 * model[5] + F.r01 * model[6] + F.r02 * model[7];
        ee[1] = F.py + F.r10 * model[5] + F.r11 * model[6] + F.r12 * model[7];
        ee[2] = F.pz + F.r20 * model[5] + F.r21 * model[6] + F.r22 * model[7];
    }
    return hit;
}

// Walks the chain at the joint values in st[0 .. A): writes the position slots, the constants' slots (velocity 0), the end
// effector, target and obstacle into the observation `o` (not with PROBE: o is unused); the DRIVEN joints' velocity slots are the
// caller's. Returns contact with the obstacle. CLEAR (the probe's walk, and the rollout step's beside its observation) also collects
// the obstacle clearance in aux.clear. CELL: the workcell is tested too (frame_geometry).
// chain_walk_at is the walk itself: joint m's value is joint(m), asked for once, in joint order, and the obstacle is given;
// st is read only for the observation (not with PROBE). chain_walk below is the walk of a pose that lies in env_state.
template <bool SC, bool PROBE, bool SCENE = false, bool CLEAR = PROBE, bool CELL = false, bool BOX = false, bool CERT = false,
          class Joint>
__device__ static inline bool chain_walk_at(const float* __restrict__ model, int A, int n_seg, const Joint& joint, float ox, float oy,
                                            float oz, float orad, const float* st, float* o, float* ee, WalkAux& aux,
                                            SceneCand* cand = nullptr) {
    const int ee_frame = (int)model[4];
    Frame F = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    ee[0] = ee[1] = ee[2] = 0.f;
    bool hit = frame_geometry<SC, PROBE, SCENE, CLEAR, CELL, BOX, CERT>(model, A, 0, F, ox, oy, oz, orad, ee_frame, ee, aux, cand);
    for (int m = 0; m < A; ++m) {
        const float* j = model + CH_HDR + m * CH_JNT;
        const float q = joint(m);
        if constexpr (!PROBE) {
            const int slot = (int)j[21];
            if (slot >= 0) o[slot] = q;
        }
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
        hit |= frame_geometry<SC, PROBE, SCENE, CLEAR, CELL, BOX, CERT>(model, A, m + 1, F, ox, oy, oz, orad, ee_frame, ee, aux, cand);
    }
    if constexpr (!PROBE) {
        const float* slots = model + ch_off_slot(A, n_seg);
        for (int k = 0; k < A; ++k)
            if (slots[2 * k] < 0.f) { o[k] = slots[2 * k + 1]; o[A + k] = 0.f; }
        for (int k = 0; k < 3; ++k) { o[2 * A + k] = ee[k]; o[2 * A + 3 + k] = st[A + k]; o[2 * A + 6 + k] = st[A + 3 + k]; }
    }
    return hit;
}

template <bool SC, bool PROBE, bool SCENE = false, bool CLEAR = PROBE, bool CELL = false, bool BOX = false>
__device__ static inline bool chain_walk(const float* __restrict__ model, int A, int n_seg, const float* st, float* o, float* ee,
                                         WalkAux& aux, SceneCand* cand = nullptr) {
    return chain_walk_at<SC, PROBE, SCENE, CLEAR, CELL, BOX>(
        model, A, n_seg, [st](int m) { return st[m]; }, st[A + 3], st[A + 4], st[A + 5], st[A + 6], st, o, ee, aux, cand);
}

// The pair phase of an SC workgroup, entered by EVERY thread after the walking wave has stored the end points: returns, to
// every thread, min over the blob's pairs of distance(segment s, segment t) - radius s - radius t for the env of its lane.
// CERT: `beta` is the lane's table of half-steps, one entry per pair; *slack receives the minimum with the pair's entry subtracted
// from every clearance, through a second row per wave behind the first.
template <bool CERT = false>
__device__ static inline float self_clearance_phase(const float* __restrict__ model, int A, int n_seg, int n_pairs, float* lds,
                                                    int lanes, int lane, bool active, const float* beta = nullptr,
                                                    float* slack = nullptr) {
    const int waves = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* segs = model + ch_off_seg(A);
    const float* pairs = model + ch_off_pair(A, n_seg);
    float* red = lds + (size_t)n_seg * 6 * lanes;
    __syncthreads();
    float best = INFINITY, low = INFINITY;
    if (active) {
        const float* ends = lds + lane;
        for (int p = wave; p < n_pairs; p += waves) {
            const int s = (int)pairs[2 * p], t = (int)pairs[2 * p + 1];
            const float* u = ends + (size_t)s * 6 * lanes;
            const float* v = ends + (size_t)t * 6 * lanes;
            const float d2 = seg_seg_dist2(u[0], u[lanes], u[2 * lanes], u[3 * lanes], u[4 * lanes], u[5 * lanes], v[0], v[lanes],
                                           v[2 * lanes], v[3 * lanes], v[4 * lanes], v[5 * lanes]);
            best = fminf(best, sqrtf(d2) - (segs[s * CH_SEG + 7] + segs[t * CH_SEG + 7]));
            if constexpr (CERT) low = fminf(low, sqrtf(d2) - (segs[s * CH_SEG + 7] + segs[t * CH_SEG + 7]) - beta[p]);
        }
        red[wave * lanes + lane] = best;
        if constexpr (CERT) red[(waves + wave) * lanes + lane] = low;
    }
    __syncthreads();
    if (active)
        for (int w = 0; w < waves; ++w) {
            best = fminf(best, red[w * lanes + lane]);
            if constexpr (CERT) low = fminf(low, red[(waves + w) * lanes + lane]);
        }
    if constexpr (CERT) *slack = low;
    return best;
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

// centre + (2u - 1) half-width of the three components: ONE rounding each, a half-width of 0 leaves the centre
__device__ static inline void scene_point(const Philox4& p, const float* centre, const float* half, float* out) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = fmaf(naf_u01(p.v[k]) * 2.f - 1.f, half[k], centre[k]);
}

// The walk of a reset pose (st[0 .. A) drawn by chain_reset_one with the same e, seed, ctr) that also chooses the episode's scene:
// the first of CH_TRIES candidates with (1) |ee - target| >= 0.05 + m, (2) clearance - obstacle radius >= m, (3) |target -
// obstacle| >= obstacle radius + 0.05 + m, else the centres. Writes the scene into st[A .. A+6) and the observation's slots.
__device__ static inline void chain_scene_walk(const float* __restrict__ model, int A, int n_seg, float* st, float* o, float* ee,
                                               WalkAux& aux, const ChainRanges& rg, int e, uint64_t seed, uint64_t ctr) {
    SceneCand cand;
#pragma unroll
    for (int c = 0; c < CH_TRIES; ++c) {
        const Philox4 p = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)e, 0x5343454Eu + 2 * c + 1, (uint32_t)seed,
                                        (uint32_t)(seed >> 32));
        scene_point(p, rg.centre + 3, rg.half + 3, cand.o[c]);
        cand.clear[c] = INFINITY;
    }
    chain_walk<false, false, true>(model, A, n_seg, st, o, ee, aux, &cand);
    const float orad = st[A + 6];
    const float far1 = CH_REACHED + rg.margin, far3 = orad + CH_REACHED + rg.margin;
    float sc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) sc[k] = rg.centre[k];
    bool found = false;
#pragma unroll
    for (int c = 0; c < CH_TRIES; ++c) {
        const Philox4 p = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)e, 0x5343454Eu + 2 * c, (uint32_t)seed,
                                        (uint32_t)(seed >> 32));
        float t[3];
        scene_point(p, rg.centre, rg.half, t);
        const float ax = ee[0] - t[0], ay = ee[1] - t[1], az = ee[2] - t[2];
        const float bx = t[0] - cand.o[c][0], by = t[1] - cand.o[c][1], bz = t[2] - cand.o[c][2];
        const bool ok = sqrtf(ax * ax + ay * ay + az * az) >= far1 && cand.clear[c] - orad >= rg.margin &&
                        sqrtf(bx * bx + by * by + bz * bz) >= far3;
        const bool take = ok && !found;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sc[k] = take ? t[k] : sc[k];
            sc[3 + k] = take ? cand.o[c][k] : sc[3 + k];
        }
        found |= ok;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) { st[A + k] = sc[k]; o[2 * A + 3 + k] = sc[k]; }
}

template <bool SCENE, class... Rg>
__global__ void __launch_bounds__(SCENE ? 64 : 1024)
chain_env_reset_kernel(const float* __restrict__ model, float* env_state, float* obs, int E, int A, int n_seg,
                                       uint64_t seed, uint64_t ctr, const ChainScene scene, const Rg... rg) {
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
    WalkAux aux = {nullptr, 0, 0.f};
    if constexpr (SCENE)
        chain_scene_walk(model, A, n_seg, st, o, ee, aux, scene_ranges(rg...), e, seed, ctr);
    else
        chain_walk<false, false>(model, A, n_seg, st, o, ee, aux);
}

// SC = false: one wave per workgroup, lane = env. SC = true: `lanes` envs per workgroup (lane < lanes of every wave), wave 0 is
// the env's walker and the only one that touches global memory; the others join it for the pair phase.
// A trailing ChainCell in the pack (CELL below): the walk of the stepped pose also tests the workcell; the walk of an auto-reset
// pose does not. The instantiations without it keep their arguments, their names and their code.
template <bool SC, bool SCENE, class... Rg>
__global__ void __launch_bounds__(SCENE ? (SC ? 64 * CH_SCENE_WAVES : 64) : 64 * CH_MAX_WAVES)
chain_env_step_kernel(const float* __restrict__ model, float* env_state, const float* __restrict__ actions,
                      float* __restrict__ out_rows, float* __restrict__ obs_next, int E, int A, int n_seg, int row_floats,
                      uint64_t seed, const uint64_t* counter_dev, int max_frames, naf_episode_record_t* __restrict__ records,
                      int record_slots, int n_pairs, int lanes, const Rg... rg) {
    constexpr bool CELL = (std::is_same_v<Rg, ChainCell> || ... || false);
    constexpr bool TAG = (std::is_same_v<Rg, ChainTag> || ... || false);
    constexpr bool BOX = (std::is_same_v<Rg, ChainBox> || ... || false);
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    int e, lane = 0;
    bool active = true, walker = true;
    if constexpr (SC) {
        lane = threadIdx.x & 63;
        e = blockIdx.x * lanes + lane;
        active = lane < lanes && e < E;
        walker = active && threadIdx.x < 64;
        if (!active) e = 0;      // (addresses below stay inside the arrays; nothing is read or written through them)
    } else {
        e = blockIdx.x * blockDim.x + threadIdx.x;
        if (e >= E) return;
    }
    const int S = 2 * A + 9;
    float* st = env_state + (int64_t)e * ch_state_floats(A);
    float* row = out_rows + (int64_t)e * row_floats;
    float* ob = obs_next + (int64_t)e * S;
    const uint64_t ctr = counter_dev ? *counter_dev : 0ull;
    const int off_s2 = naf_row_off_s2(S, A), off_d = naf_row_off_done(S, A);
    float* o2 = row + off_s2;
    float ee[3];
    bool hit = false;
    WalkAux aux = {SC ? ch_lds + lane : nullptr, lanes, 0.f};

    if (walker) {
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
        hit = chain_walk<SC, false, false, false, CELL, BOX>(model, A, n_seg, st, o2, ee, aux);
    }
    if constexpr (SC) {
        // self-contact counts as contact (environment.py:311-343); the walker's lanes hold the minimum over all pairs
        const float self_clear = self_clearance_phase(model, A, n_seg, n_pairs, ch_lds, lanes, lane, active);
        if (!walker) return;
        hit |= self_clear < 0.f;
    }
    float dx = ee[0] - st[A], dy = ee[1] - st[A + 1], dz = ee[2] - st[A + 2];
    float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    const bool reached = dist < 0.05f;
    float reward = reached ? 250.f : (hit ? -1000.f : -(dist - 0.05f));
    float done = (reached || hit) ? 1.f : 0.f;
    row[S + A] = reward;
    for (int k = S + A + 1; k < off_s2; ++k) row[k] = 0.f;
    row[off_d] = done;
    for (int k = off_d + 1; k < row_floats; ++k) row[k] = 0.f;
    if constexpr (TAG) row[row_floats - 1] = st[A + 8] + 1.f;      // rec.episode below; the host checked row_floats - 1 > off_d

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
        if constexpr (SCENE)
            chain_scene_walk(model, A, n_seg, st, ob, ee, aux, scene_ranges(rg...), e, seed,
                             ctr * 0x9E3779B97F4A7C15ull + (uint64_t)st[A + 8]);
        else
            chain_walk<false, false>(model, A, n_seg, st, ob, ee, aux);
    } else {
        for (int k = 0; k < S; ++k) ob[k] = o2[k];
    }
}

// naf_chain_env_probe_cell: the workcell clearance of the pose in env_state. One wave per workgroup, lane = env: the workcell needs
// no pair phase.
__global__ void __launch_bounds__(64)
chain_env_probe_cell_kernel(const float* __restrict__ model, const float* __restrict__ env_state, float* __restrict__ out, int E, int A,
                            int n_seg) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float ee[3];
    WalkAux aux = {nullptr, 0, INFINITY, INFINITY};
    chain_walk<false, true, false, true, true>(model, A, n_seg, env_state + (int64_t)e * ch_state_floats(A), nullptr, ee, aux);
    out[e] = aux.cell;
}

// the same for a model with boxes
__global__ void __launch_bounds__(64)
chain_env_probe_cell_box_kernel(const float* __restrict__ model, const float* __restrict__ env_state, float* __restrict__ out, int E,
                                int A, int n_seg) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float ee[3];
    WalkAux aux = {nullptr, 0, INFINITY, INFINITY};
    chain_walk<false, true, false, true, true, true>(model, A, n_seg, env_state + (int64_t)e * ch_state_floats(A), nullptr, ee, aux);
    out[e] = aux.cell;
}

// naf_chain_env_probe: the walk and the pair phase of the step at the joint values in env_state, nothing written but `out`
template <bool SC>
__global__ void __launch_bounds__(64 * CH_MAX_WAVES)
chain_env_probe_kernel(const float* __restrict__ model, const float* __restrict__ env_state, float* __restrict__ out, int E, int A,
                       int n_seg, int n_pairs, int lanes) {
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    int e, lane = 0;
    bool active = true, walker = true;
    if constexpr (SC) {
        lane = threadIdx.x & 63;
        e = blockIdx.x * lanes + lane;
        active = lane < lanes && e < E;
        walker = active && threadIdx.x < 64;
        if (!active) e = 0;
    } else {
        e = blockIdx.x * blockDim.x + threadIdx.x;
        if (e >= E) return;
    }
    const float* st = env_state + (int64_t)e * ch_state_floats(A);
    float ee[3];
    WalkAux aux = {SC ? ch_lds + lane : nullptr, lanes, INFINITY};
    if (walker) chain_walk<SC, true>(model, A, n_seg, st, nullptr, ee, aux);
    float self_clear = INFINITY;
    if constexpr (SC) {
        self_clear = self_clearance_phase(model, A, n_seg, n_pairs, ch_lds, lanes, lane, active);
        if (!walker) return;
    }
    float* o = out + (int64_t)e * NAF_CHAIN_PROBE_FLOATS;
    o[0] = ee[0]; o[1] = ee[1]; o[2] = ee[2];
    o[3] = aux.clear - st[A + 6];
    o[4] = self_clear;
}

// naf_chain_env_reset_given: env e starts at q0[e] (clamped into the limits as a step clamps) in the scene scene[e]; nothing is drawn
__global__ void __launch_bounds__(64)
chain_env_reset_given_kernel(const float* __restrict__ model, float* env_state, float* obs, int E, int A, int n_seg,
                             const float* __restrict__ q0, const float* __restrict__ scene, float orad) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int nst = ch_state_floats(A);
    float* st = env_state + (int64_t)e * nst;
    float* o = obs + (int64_t)e * (2 * A + 9);
    for (int k = A; k < nst; ++k) st[k] = 0.f;
    for (int k = 0; k < 6; ++k) st[A + k] = scene[(int64_t)e * 6 + k];
    st[A + 6] = orad;
    for (int m = 0; m < A; ++m) {
        const float* j = model + CH_HDR + m * CH_JNT;
        float q = q0[(int64_t)e * A + m];
        if (j[16] != 0.f) {
            if (q > j[18]) q = j[18];
            if (q < j[17]) q = j[17];
        }
        st[m] = q;
        const int slot = (int)j[21];
        if (slot >= 0) o[A + slot] = 0.f;
    }
    float ee[3];
    WalkAux aux = {nullptr, 0, 0.f};
    chain_walk<false, false>(model, A, n_seg, st, o, ee, aux);
}

// naf_chain_env_rollout_step: the step kernel's tick for a query instead of a training stream. An env whose episode is over
// (env_state[A+8] >= 1) is HELD: its lane walks nothing and writes nothing, and in an SC workgroup only joins the barriers. A live
// lane writes the observation straight into obs_next, keeps its outcome record and, with traj, its joint values of the frame.
// A trailing ChainCell (CELL below, as in chain_env_step_kernel): code 4 and outcome[6], the workcell's.
template <bool SC, class... Cell>
__global__ void __launch_bounds__(SC ? 64 * CH_MAX_WAVES : 64)      // (without SC a workgroup is one wave)
chain_env_rollout_kernel(const float* __restrict__ model, float* env_state, const float* __restrict__ actions,
                         float* __restrict__ obs_next, float* __restrict__ outcome, float* __restrict__ traj, int E, int A, int n_seg,
                         int max_frames, int n_pairs, int lanes, const Cell... cell) {
    constexpr bool CELL = (std::is_same_v<Cell, ChainCell> || ... || false);
    constexpr bool BOX = (std::is_same_v<Cell, ChainBox> || ... || false);
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    int e, lane = 0;
    bool active = true, walker = true;
    if constexpr (SC) {
        lane = threadIdx.x & 63;
        e = blockIdx.x * lanes + lane;
        active = lane < lanes && e < E;
        walker = active && threadIdx.x < 64;
        if (!active) e = 0;      // (addresses below stay inside the arrays; nothing is written through them)
    } else {
        e = blockIdx.x * blockDim.x + threadIdx.x;
        if (e >= E) return;
    }
    const int S = 2 * A + 9;
    float* st = env_state + (int64_t)e * ch_state_floats(A);
    float* ob = obs_next + (int64_t)e * S;
    // every wave of an SC workgroup reads the hold flag here, before the first barrier; the walker raises it behind the second
    const bool live = active && st[A + 8] < 1.f;
    walker = walker && live;
    if constexpr (!SC)
        if (!live) return;
    float ee[3];
    bool hit = false;
    WalkAux aux = {SC ? ch_lds + lane : nullptr, lanes, INFINITY, INFINITY};
    if (walker) {
        for (int m = 0; m < A; ++m) {
            const float* j = model + CH_HDR + m * CH_JNT;
            const float a = actions[(int64_t)e * A + m];
            float q = st[m] + CH_DT * a;      // the step kernel's rule: velocity control, then the position limits
            float vel = a;
            if (j[16] != 0.f) {
                if (q > j[18]) { q = j[18]; vel = 0.f; }
                if (q < j[17]) { q = j[17]; vel = 0.f; }
            }
            st[m] = q;
            const int slot = (int)j[21];
            if (slot >= 0) ob[A + slot] = vel;
        }
        hit = chain_walk<SC, false, false, true, CELL, BOX>(model, A, n_seg, st, ob, ee, aux);
    }
    float self_clear = INFINITY;
    if constexpr (SC) {
        self_clear = self_clearance_phase(model, A, n_seg, n_pairs, ch_lds, lanes, lane, live);
        if (!walker) return;
    }
    const bool self_hit = self_clear < 0.f;
    const bool cell_hit = CELL && aux.cell < 0.f;
    float dx = ee[0] - st[A], dy = ee[1] - st[A + 1], dz = ee[2] - st[A + 2];
    float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    const bool reached = dist < 0.05f;
    const float reward = reached ? 250.f : ((hit || self_hit || cell_hit) ? -1000.f : -(dist - 0.05f));
    const bool done = reached || hit || self_hit || cell_hit;
    const bool first = st[A + 7] == 0.f;
    const float frame = st[A + 7] + 1.f;
    st[A + 7] = frame;
    double* score_p = (double*)(st + ch_off_score(A));
    const double score = *score_p + (double)reward;
    *score_p = score;
    float* oc = outcome + (int64_t)e * NAF_CHAIN_OUTCOME_FLOATS;
    oc[0] = reached ? 1.f : (hit ? 2.f : (self_hit ? 3.f : (cell_hit ? 4.f : 0.f)));
    oc[1] = frame;
    oc[2] = dist;
    oc[3] = fminf(first ? INFINITY : oc[3], aux.clear - st[A + 6]);
    oc[4] = fminf(first ? INFINITY : oc[4], self_clear);
    oc[5] = (float)score;
    if constexpr (CELL) oc[6] = fminf(first ? INFINITY : oc[6], aux.cell);
    else oc[6] = 0.f;
    oc[7] = 0.f;
    if (traj && frame <= (float)max_frames) {      // (a record that did not come from reset_given cannot write past the buffer)
        float* tr = traj + ((int64_t)frame * E + e) * A;
        for (int m = 0; m < A; ++m) tr[m] = st[m];
    }
    if (done || frame >= (float)max_frames) st[A + 8] += 1.f;
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
    if (!ch_int(m[8], CH_HDR, 1 << 24, &total) || total != n_floats) return NAF_CHAIN_ERR_SIZE;
    int P = 0, G = 0, H = 0, B = 0;
    const bool pairs_counted = ch_int(m[9], 0, 1 << 22, &P);
    // (a blob without a workcell has zeros here and takes every check below as it always did)
    if (!ch_int(m[10], 0, NAF_CHAIN_MAX_CELL, &G) || !ch_int(m[11], 0, NAF_CHAIN_MAX_CELL - G, &H) ||
        !ch_int(m[12], 0, NAF_CHAIN_MAX_CELL - G - H, &B))
        return NAF_CHAIN_ERR_CELL;
    const int cell = G + H + B > 0 ? 4 * (G + H) + CH_BOX * B + n_seg : 0;
    if (pairs_counted && P == 0 && cell == 0 && total != ch_off_pair(A, n_seg)) return NAF_CHAIN_ERR_SIZE;
    for (int k = 0; k < n_floats; ++k)
        if (!std::isfinite(m[k])) return NAF_CHAIN_ERR_VALUE;
    if (!pairs_counted || (cell == 0 && total != ch_off_pair(A, n_seg) + 2 * P)) return NAF_CHAIN_ERR_PAIRS;
    if (cell > 0 && (int64_t)total != (int64_t)ch_off_cell(A, n_seg, P) + cell) return NAF_CHAIN_ERR_CELL;
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
    const float* pairs = m + ch_off_pair(A, n_seg);
    std::vector<int64_t> seen;
    seen.reserve(P);
    for (int p = 0; p < P; ++p) {
        int s, t;
        if (!ch_int(pairs[2 * p], 0, n_seg - 1, &s) || !ch_int(pairs[2 * p + 1], s + 1, n_seg - 1, &t)) return NAF_CHAIN_ERR_PAIRS;
        seen.push_back((int64_t)s * n_seg + t);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return NAF_CHAIN_ERR_PAIRS;
    const float* geo = m + ch_off_cell(A, n_seg, P);
    for (int g = 0; g < G; ++g)
        if (geo[4 * g + 3] < 0.f) return NAF_CHAIN_ERR_CELL;
    for (int g = G; g < G + H; ++g) {
        const float* n = geo + 4 * g;
        if (std::fabs(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] - 1.f) > 1e-4f) return NAF_CHAIN_ERR_CELL;
    }
    for (int b = 0; b < B; ++b) {
        const float* x = geo + 4 * (G + H) + CH_BOX * b;      // c | R row-major | h | r
        const float* R = x + 3;
        if (x[12] < 0.f || x[13] < 0.f || x[14] < 0.f || x[15] < 0.f) return NAF_CHAIN_ERR_CELL;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const float dot = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2];
                if (std::fabs(dot - (i == j ? 1.f : 0.f)) > 1e-4f) return NAF_CHAIN_ERR_CELL;
            }
    }
    for (int s = 0; cell > 0 && s < n_seg; ++s) {
        int mask;
        if (!ch_int(geo[4 * (G + H) + CH_BOX * B + s], 0, (1 << (G + H + B)) - 1, &mask)) return NAF_CHAIN_ERR_CELL;
    }
    return NAF_OK;
}

// ---- how a handle's model is launched --------------------------------------------------------------------------------------------
// Three things, each stated here once; the entry points below are their argument checks and one launch expression through them.
// ch_with_cell: the pack a model's kernels take behind their fixed arguments. ch_with_pack: std::true_type in front of it for a
// model with collision pairs (the kernels' SC). A launch with more in its pack puts it around these: ChainRanges in front and
// ChainTag behind in the step, ChainCert in front in the certifying launch.
template <class F>
static int ch_with_cell(const naf_chain_env* h, F&& f) {
    if (h->n_box > 0) return f(ChainCell{}, ChainBox{});
    if (h->n_cell > 0) return f(ChainCell{});
    return f();
}
template <class F>
static int ch_with_sc(const naf_chain_env* h, F&& f) {
    return h->n_pairs > 0 ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
static int ch_with_pack(const naf_chain_env* h, F&& f) {
    return ch_with_sc(h, [&](auto sc) { return ch_with_cell(h, [&](auto... cell) { return f(sc, cell...); }); });
}

// The launch shape that goes with SC: workgroup size, dynamic LDS, the kernels' n_pairs and lanes arguments, the grid for E envs.
// Without pairs a workgroup is one wave of 64 envs and has no LDS.
struct ChShape {
    unsigned block;
    size_t lds;
    int n_pairs, lanes;
    unsigned grid(int E) const { return (unsigned)((E + lanes - 1) / lanes); }
};
template <bool SC>
static ChShape ch_shape(const naf_chain_env* h, int waves) {
    if constexpr (SC) return {64u * waves, ch_lds_bytes(h->n_seg, h->lanes, waves), h->n_pairs, h->lanes};
    return {64u, 0, 0, 64};
}

// Kernel K's dynamic LDS may exceed the 64 KB a kernel gets unasked: raised once per device, and the flag is K's own
template <auto K>
static int ch_raise(int bytes = CH_MAX_DYN_LDS) {
    static bool raised_dev[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 0 || dev >= 64) return NAF_ERR_ARG;
    if (raised_dev[dev]) return NAF_OK;
    e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    raised_dev[dev] = true;
    return NAF_OK;
}

// One launch of kernel K in shape w. The kernels whose launches engine.py captures into graphs (step, probe, rollout) go through
// this one: naf_chain_env_create raised their limits, and nothing here calls the runtime but the launch.
template <auto K, class... Args>
static int ch_launch(unsigned grid, const ChShape& w, void* stream, Args... args) {
    K<<<grid, w.block, w.lds, (hipStream_t)stream>>>(args...);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}
// The same for an entry point no graph captures (path, certify, demonstrations): an SC launch first raises K's limit to `bytes`
template <auto K, class... Args>
static int ch_launch_raising(int bytes, unsigned grid, const ChShape& w, void* stream, Args... args) {
    if (w.n_pairs > 0) {
        const int rc = ch_raise<K>(bytes);
        if (rc != NAF_OK) return rc;
    }
    return ch_launch<K>(grid, w, stream, args...);
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
    h->n_pairs = (int)model_host[9];
    h->n_box = (int)model_host[12];
    h->ee_frame = (int)model_host[4];
    h->n_cell = (int)model_host[10] + (int)model_host[11] + h->n_box;
    h->lanes = 64;
    h->waves = 1;
    if (h->n_pairs > 0) {
        // fewer envs per workgroup for an arm whose end points do not fit with 64; a refusal when one env's do not fit
        h->waves = std::min(CH_MAX_WAVES, (h->n_pairs + CH_PAIRS_PER_WAVE - 1) / CH_PAIRS_PER_WAVE);
        while (h->lanes > 1 && ch_lds_bytes(h->n_seg, h->lanes, h->waves) > CH_MAX_DYN_LDS) h->lanes >>= 1;
        rc = ch_lds_bytes(h->n_seg, h->lanes, h->waves) > CH_MAX_DYN_LDS ? NAF_CHAIN_ERR_LDS : NAF_OK;
        // raised here, eagerly, for the kernels whose launches are captured into graphs: this handle's own step, probe and rollout
        if (rc == NAF_OK)
            rc = ch_with_cell(h, [](auto... cell) {
                int r = ch_raise<chain_env_step_kernel<true, false, decltype(cell)...>>();
                if (r == NAF_OK) r = ch_raise<chain_env_step_kernel<true, true, ChainRanges, decltype(cell)...>>();
                if (r == NAF_OK) r = ch_raise<chain_env_step_kernel<true, false, decltype(cell)..., ChainTag>>();
                if (r == NAF_OK) r = ch_raise<chain_env_step_kernel<true, true, ChainRanges, decltype(cell)..., ChainTag>>();
                if (r == NAF_OK) r = ch_raise<chain_env_probe_kernel<true>>();
                if (r == NAF_OK) r = ch_raise<chain_env_rollout_kernel<true, decltype(cell)...>>();
                return r;
            });
        if (rc != NAF_OK) {
            delete h;
            return rc;
        }
    }
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

extern "C" int naf_chain_env_set_scene_ranges(naf_chain_env_t* h, const float* ranges_host) {
    if (!h) return NAF_ERR_ARG;
    bool on = false;
    for (int k = 0; ranges_host && k < NAF_CHAIN_RANGE_FLOATS; ++k) {
        if (!std::isfinite(ranges_host[k]) || ranges_host[k] < 0.f) return NAF_ERR_ARG;
        on |= k < 6 && ranges_host[k] > 0.f;
    }
    for (int k = 0; k < NAF_CHAIN_RANGE_FLOATS; ++k) h->ranges[k] = ranges_host ? ranges_host[k] : 0.f;
    h->scene_on = on;
    h->scene_ready = false;
    return NAF_OK;
}

static ChainRanges ch_ranges(const naf_chain_env* h) {
    ChainRanges rg;
    for (int k = 0; k < 6; ++k) { rg.centre[k] = h->centre[k]; rg.half[k] = h->ranges[k]; }
    rg.margin = h->ranges[6];
    return rg;
}

extern "C" int naf_chain_env_reset(naf_chain_env_t* h, float* env_state, float* obs, int E, const float* scene_host, uint64_t seed,
                                   uint64_t counter, void* stream) {
    if (!h || !env_state || !obs || !scene_host || E <= 0) return NAF_ERR_ARG;
    ChainScene sc;
    for (int k = 0; k < NAF_CHAIN_SCENE_FLOATS; ++k) sc.v[k] = scene_host[k];
    if (!(sc.v[7] >= 0.f) || !(sc.v[6] >= 0.f)) return NAF_ERR_ARG;
    if (h->scene_on) {
        if (sc.v[6] != 0.f) return NAF_ERR_ARG;      // the jitter is drawn once per env, the scene every episode: one or the other
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(sc.v[k])) return NAF_ERR_ARG;
        for (int k = 0; k < 6; ++k) h->centre[k] = sc.v[k];
        h->scene_ready = true;
        chain_env_reset_kernel<true, ChainRanges><<<(E + 63) / 64, 64, 0, (hipStream_t)stream>>>(h->model_dev, env_state, obs, E, h->A, h->n_seg,
                                                                                    seed, counter, sc, ch_ranges(h));
    } else
        chain_env_reset_kernel<false><<<(E + 63) / 64, 64, 0, (hipStream_t)stream>>>(h->model_dev, env_state, obs, E, h->A, h->n_seg,
                                                                                     seed, counter, sc);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

// Tag: nothing (naf_chain_env_step: the launches are the ones they always were) or one ChainTag (naf_chain_env_step_tagged).
// The scene choice is the step's own: ChainRanges leads the pack of a SCENE launch, whose workgroups are at most CH_SCENE_WAVES waves.
template <class... Tag>
static int ch_step_launch(naf_chain_env_t* h, float* env_state, const float* actions, float* out_rows, float* obs_next,
                          int E, uint64_t seed, const uint64_t* counter_dev, int max_frames, naf_episode_record_t* records,
                          int record_slots, void* stream, const Tag... tag) {
    if (!h || !env_state || !actions || !out_rows || !obs_next || E <= 0) return NAF_ERR_ARG;
    if (records && (record_slots <= 0 || !counter_dev)) return NAF_ERR_ARG;
    const int rf = naf_replay_row_floats(2 * h->A + 9, h->A);
    if (rf <= 0) return NAF_ERR_ARG;
    if (h->scene_on && !h->scene_ready) return NAF_ERR_STATE;
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        const ChShape w = ch_shape<sc()>(h, h->scene_on ? std::min(h->waves, CH_SCENE_WAVES) : h->waves);
        auto launch = [&](auto scene, auto... rg) {
            return ch_launch<chain_env_step_kernel<sc(), scene(), decltype(rg)..., decltype(cell)..., Tag...>>(
                w.grid(E), w, stream, h->model_dev, env_state, actions, out_rows, obs_next, E, h->A, h->n_seg, rf, seed, counter_dev,
                max_frames, records, record_slots, w.n_pairs, w.lanes, rg..., cell..., tag...);
        };
        return h->scene_on ? launch(std::true_type{}, ch_ranges(h)) : launch(std::false_type{});
    });
}

extern "C" int naf_chain_env_step(naf_chain_env_t* h, float* env_state, const float* actions, float* out_rows, float* obs_next,
                                  int E, uint64_t seed, const uint64_t* counter_dev, int max_frames, naf_episode_record_t* records,
                                  int record_slots, void* stream) {
    return ch_step_launch(h, env_state, actions, out_rows, obs_next, E, seed, counter_dev, max_frames, records, record_slots, stream);
}

// the same step; every row's last float (naf_replay_row_floats - 1) holds the episode ordinal its record reports
extern "C" int naf_chain_env_step_tagged(naf_chain_env_t* h, float* env_state, const float* actions, float* out_rows,
                                         float* obs_next, int E, uint64_t seed, const uint64_t* counter_dev, int max_frames,
                                         naf_episode_record_t* records, int record_slots, void* stream) {
    if (!h) return NAF_ERR_ARG;
    const int S = 2 * h->A + 9;
    // the tag needs a float of the padded row that the learner's minibatch row does not reach (none at A = 21 and A = 47)
    if (naf_replay_row_floats(S, h->A) - 1 < naf_replay_batch_row_floats(S, h->A)) return NAF_ERR_ARG;
    return ch_step_launch(h, env_state, actions, out_rows, obs_next, E, seed, counter_dev, max_frames, records, record_slots, stream,
                          ChainTag{});
}

extern "C" int naf_chain_env_probe(naf_chain_env_t* h, const float* env_state, float* out, int E, void* stream) {
    if (!h || !env_state || !out || E <= 0) return NAF_ERR_ARG;
    return ch_with_sc(h, [&](auto sc) {
        const ChShape w = ch_shape<sc()>(h, h->waves);
        return ch_launch<chain_env_probe_kernel<sc()>>(w.grid(E), w, stream, h->model_dev, env_state, out, E, h->A, h->n_seg, w.n_pairs,
                                                       w.lanes);
    });
}

extern "C" int naf_chain_env_probe_cell(naf_chain_env_t* h, const float* env_state, float* out, int E, void* stream) {
    if (!h || !env_state || !out || E <= 0) return NAF_ERR_ARG;
    if (h->n_cell == 0) return NAF_ERR_STATE;
    const ChShape w = ch_shape<false>(h, 1);      // one wave per workgroup: the workcell needs no pair phase
    if (h->n_box > 0) return ch_launch<chain_env_probe_cell_box_kernel>(w.grid(E), w, stream, h->model_dev, env_state, out, E, h->A, h->n_seg);
    return ch_launch<chain_env_probe_cell_kernel>(w.grid(E), w, stream, h->model_dev, env_state, out, E, h->A, h->n_seg);
}

extern "C" int naf_chain_env_reset_given(naf_chain_env_t* h, float* env_state, float* obs, int E, const float* q0_dev,
                                         const float* scene_dev, float obstacle_radius, void* stream) {
    if (!h || !env_state || !obs || !q0_dev || !scene_dev || E <= 0 || !(obstacle_radius >= 0.f)) return NAF_ERR_ARG;
    chain_env_reset_given_kernel<<<(E + 63) / 64, 64, 0, (hipStream_t)stream>>>(h->model_dev, env_state, obs, E, h->A, h->n_seg, q0_dev,
                                                                                scene_dev, obstacle_radius);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

extern "C" int naf_chain_env_rollout_step(naf_chain_env_t* h, float* env_state, const float* actions, float* obs_next, float* outcome,
                                          float* traj, int E, int max_frames, void* stream) {
    if (!h || !env_state || !actions || !obs_next || !outcome || E <= 0 || max_frames < 1) return NAF_ERR_ARG;
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        const ChShape w = ch_shape<sc()>(h, h->waves);
        return ch_launch<chain_env_rollout_kernel<sc(), decltype(cell)...>>(w.grid(E), w, stream, h->model_dev, env_state, actions, obs_next,
                                                                            outcome, traj, E, h->A, h->n_seg, max_frames, w.n_pairs,
                                                                            w.lanes, cell...);
    });
}

// ---- goal poses: damped least squares on the end effector's positional Jacobian (include/naf_hip.h, "Goal poses") ----------------
// One lane per candidate (query n, restart r), the R candidates of a query in adjacent lanes, one wave per workgroup: no barrier
// anywhere, an inactive tail lane returns at once. The pose lives in q_out (read and written as the walk and the update reach each
// joint, as the step kernels keep theirs in env_state); the walk leaves every driven joint's world axis a_m and a point p_m on
// it in LDS as [m][6][lane] floats — lane-contiguous, conflict-free, and no per-lane array is indexed at run time. Each lane
// reads back only what it wrote. Joints behind the end-effector frame are not walked: their columns are 0.

// walks joints 0 .. ee_frame - 1 at the joint values q; STORE: a_m | p_m to ax[(m * 6 + k) * 64]; returns the end effector in ee
// and, with ROT, the end frame's rotation R_ee in rot[9], row-major. MID: the walk is at the middle (q + q2) / 2 of two poses,
// formed joint by joint as the walk reaches it — no pose array of the lane's own
template <bool STORE, bool ROT = false, bool MID = false>
__device__ static inline void ik_walk(const float* __restrict__ model, int n_joints, const float* q, float* ax, float* ee,
                                      float* rot = nullptr, const float* q2 = nullptr) {
    Frame F = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < n_joints; ++m) {
        const float* j = model + CH_HDR + m * CH_JNT;
        float qm = q[m];
        if constexpr (MID) qm = (qm + q2[m]) * 0.5f;
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
        const float wx = G.r00 * x + G.r01 * y + G.r02 * z, wy = G.r10 * x + G.r11 * y + G.r12 * z,
                    wz = G.r20 * x + G.r21 * y + G.r22 * z;
        if constexpr (STORE) {
            float* w = ax + m * 6 * 64;
            w[0] = wx; w[64] = wy; w[128] = wz;
            w[192] = F.px; w[256] = F.py; w[320] = F.pz;
        }
        if (j[15] != 0.f) {      // prismatic
            F.r00 = G.r00; F.r01 = G.r01; F.r02 = G.r02;
            F.r10 = G.r10; F.r11 = G.r11; F.r12 = G.r12;
            F.r20 = G.r20; F.r21 = G.r21; F.r22 = G.r22;
            F.px += wx * qm;
            F.py += wy * qm;
            F.pz += wz * qm;
        } else {                 // revolute: chain_walk's Rodrigues form
            float s, c;
            sincosf(qm, &s, &c);
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
    }
    ee[0] = F.px + F.r00 * model[5] + F.r01 * model[6] + F.r02 * model[7];
    ee[1] = F.py + F.r10 * model[5] + F.r11 * model[6] + F.r12 * model[7];
    ee[2] = F.pz + F.r20 * model[5] + F.r21 * model[6] + F.r22 * model[7];
    if constexpr (ROT) {
        rot[0] = F.r00; rot[1] = F.r01; rot[2] = F.r02;
        rot[3] = F.r10; rot[4] = F.r11; rot[5] = F.r12;
        rot[6] = F.r20; rot[7] = F.r21; rot[8] = F.r22;
    }
}

// Jacobian column of joint m from its LDS record: a x (ee - p), or a for a prismatic joint
__device__ static inline void ik_column(const float* __restrict__ model, int m, const float* ax, const float* ee, float* c) {
    const float* w = ax + m * 6 * 64;
    const float a0 = w[0], a1 = w[64], a2 = w[128];
    if (model[CH_HDR + m * CH_JNT + 15] != 0.f) {
        c[0] = a0; c[1] = a1; c[2] = a2;
    } else {
        const float d0 = ee[0] - w[192], d1 = ee[1] - w[256], d2 = ee[2] - w[320];
        c[0] = a1 * d2 - a2 * d1;
        c[1] = a2 * d0 - a0 * d2;
        c[2] = a0 * d1 - a1 * d0;
    }
}

// The frame the two solve kernels share. ik_seed: candidate cand = (query n, restart r) starts from q_start[n] (r = 0) or from its
// seed, copied into its place in q_out, which is returned. REC: iters_out [K + 1][N R][A] receives the pose before the first and
// after every update.
template <bool REC>
__device__ __forceinline__ float* ik_seed(const float* __restrict__ q_start, const float* __restrict__ seeds, int64_t cand, int64_t n,
                                          int R, int A, float* q_out, float* __restrict__ iters_out) {
    const int r = (int)(cand - n * R);
    float* q = q_out + cand * A;
    const float* src = r == 0 ? q_start + n * A : seeds + cand * A;
    for (int m = 0; m < A; ++m) {
        const float v = src[m];
        q[m] = v;
        if constexpr (REC) iters_out[cand * A + m] = v;
    }
    return q;
}

// ik_update: q_m += scale dq_m for the walked joints (pass 2 left dq_m in the LDS record's first float), then the position
// limits, as a step applies them. REC: the pose also goes to `rec`, the candidate's place in the update's slab of iters_out.
template <bool REC>
__device__ __forceinline__ void ik_update(const float* __restrict__ model, int n_joints, int A, float scale, const float* ax, float* q,
                                          float* __restrict__ rec) {
    for (int m = 0; m < A; ++m) {
        const float* j = model + CH_HDR + m * CH_JNT;
        float v = q[m];
        if (m < n_joints) v += scale * ax[m * 6 * 64];
        if (j[16] != 0.f) {
            if (v > j[18]) v = j[18];
            if (v < j[17]) v = j[17];
        }
        q[m] = v;
        if constexpr (REC) rec[m] = v;
    }
}

// chain_ik_solve_kernel's update between its walk and ik_update, restated for chain_line_track_kernel expression for expression
// (calling it from the solve kernel changed that kernel's code beyond scheduling, so the solve kernel keeps its own text): from the
// walk's LDS record and ee towards (g0, g1, g2) it leaves dq_m in the record's first float and returns the dq_max scale
__device__ __forceinline__ float ik_delta(const float* __restrict__ model, int n_joints, float* ax, const float* ee, float g0, float g1,
                                          float g2, const naf_chain_ik_params_t& prm) {
    float e0 = g0 - ee[0], e1 = g1 - ee[1], e2 = g2 - ee[2];
    const float len = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    if (len > prm.e_max) {
        const float s = prm.e_max / len;
        e0 *= s; e1 *= s; e2 *= s;
    }
    // pass 1 over LDS: M = sum c c^T + lam^2 I
    float m00 = prm.lam2, m01 = 0.f, m02 = 0.f, m11 = prm.lam2, m12 = 0.f, m22 = prm.lam2;
    for (int m = 0; m < n_joints; ++m) {
        float c[3];
        ik_column(model, m, ax, ee, c);
        m00 += c[0] * c[0]; m01 += c[0] * c[1]; m02 += c[0] * c[2];
        m11 += c[1] * c[1]; m12 += c[1] * c[2]; m22 += c[2] * c[2];
    }
    // M y = e in closed form: the adjugate over the determinant
    const float c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const float c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const float det = m00 * c00 + m01 * c01 + m02 * c02;
    const float y0 = (c00 * e0 + c01 * e1 + c02 * e2) / det, y1 = (c01 * e0 + c11 * e1 + c12 * e2) / det,
                y2 = (c02 * e0 + c12 * e1 + c22 * e2) / det;
    // pass 2: dq_m = c_m . y, kept in the record's first float, and max |dq_m|
    float big = 0.f;
    for (int m = 0; m < n_joints; ++m) {
        float c[3];
        ik_column(model, m, ax, ee, c);
        const float dq = c[0] * y0 + c[1] * y1 + c[2] * y2;
        ax[m * 6 * 64] = dq;
        big = fmaxf(big, fabsf(dq));
    }
    return big > prm.dq_max ? prm.dq_max / big : 1.f;
}

template <bool REC>
__global__ void __launch_bounds__(64)
chain_ik_solve_kernel(const float* __restrict__ model, const float* __restrict__ targets, const float* __restrict__ q_start,
                      const float* __restrict__ seeds, int N, int R, int A, const naf_chain_ik_params_t prm, float* q_out,
                      float* __restrict__ residual_out, float* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    const int64_t total = (int64_t)N * R;
    const int64_t cand = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (cand >= total) return;      // (one wave per workgroup and no barrier below)
    const int64_t n = cand / R;
    const int n_joints = (int)model[4];      // the end-effector frame: joints m >= it do not move the end effector
    float* ax = ch_lds + threadIdx.x;
    float* q = ik_seed<REC>(q_start, seeds, cand, n, R, A, q_out, iters_out);
    const float g0 = targets[n * 3], g1 = targets[n * 3 + 1], g2 = targets[n * 3 + 2];
    float ee[3];
    for (int k = 0; k < prm.iterations; ++k) {
        ik_walk<true>(model, n_joints, q, ax, ee);
        float e0 = g0 - ee[0], e1 = g1 - ee[1], e2 = g2 - ee[2];
        const float len = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
        if (len > prm.e_max) {
            const float s = prm.e_max / len;
            e0 *= s; e1 *= s; e2 *= s;
        }
        // pass 1 over LDS: M = sum c c^T + lam^2 I
        float m00 = prm.lam2, m01 = 0.f, m02 = 0.f, m11 = prm.lam2, m12 = 0.f, m22 = prm.lam2;
        for (int m = 0; m < n_joints; ++m) {
            float c[3];
            ik_column(model, m, ax, ee, c);
            m00 += c[0] * c[0]; m01 += c[0] * c[1]; m02 += c[0] * c[2];
            m11 += c[1] * c[1]; m12 += c[1] * c[2]; m22 += c[2] * c[2];
        }
        // M y = e in closed form: the adjugate over the determinant
        const float c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
        const float c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const float det = m00 * c00 + m01 * c01 + m02 * c02;
        const float y0 = (c00 * e0 + c01 * e1 + c02 * e2) / det, y1 = (c01 * e0 + c11 * e1 + c12 * e2) / det,
                    y2 = (c02 * e0 + c12 * e1 + c22 * e2) / det;
        // pass 2: dq_m = c_m . y, kept in the record's first float, and max |dq_m|
        float big = 0.f;
        for (int m = 0; m < n_joints; ++m) {
            float c[3];
            ik_column(model, m, ax, ee, c);
            const float dq = c[0] * y0 + c[1] * y1 + c[2] * y2;
            ax[m * 6 * 64] = dq;
            big = fmaxf(big, fabsf(dq));
        }
        const float scale = big > prm.dq_max ? prm.dq_max / big : 1.f;
        ik_update<REC>(model, n_joints, A, scale, ax, q, REC ? iters_out + ((int64_t)(k + 1) * total + cand) * A : nullptr);
    }
    ik_walk<false>(model, n_joints, q, ax, ee);
    const float e0 = g0 - ee[0], e1 = g1 - ee[1], e2 = g2 - ee[2];
    residual_out[cand] = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
}

// The selection among the R adjacent lanes of a query: key (class, joint distance or residual, r), a butterfly of shuffles
// inside the group. A group lies inside one wave and is active or inactive as a whole (R divides 64).
__global__ void __launch_bounds__(64)
chain_ik_select_kernel(const float* __restrict__ q_out, const float* __restrict__ q_start, const float* __restrict__ residual,
                       const float* __restrict__ probe, const float* __restrict__ cell, int N, int R, int A, float tolerance,
                       float margin, int* __restrict__ choice_out, int* __restrict__ class_out, float* __restrict__ jd_out) {
    const int64_t total = (int64_t)N * R;
    int64_t cand = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool active = cand < total;
    if (!active) cand = 0;      // (addresses stay inside the arrays; nothing is written through them)
    const int64_t n = cand / R;
    int r = (int)(cand - n * R);
    float jd = 0.f;
    for (int m = 0; m < A; ++m) jd = fmaxf(jd, fabsf(q_out[cand * A + m] - q_start[n * A + m]));
    const float res = residual[cand];
    const float* p = probe + cand * NAF_CHAIN_PROBE_FLOATS;
    const bool free_ = p[3] >= margin && p[4] >= margin && (!cell || cell[cand] >= margin);
    int cls = res <= tolerance ? (free_ ? 0 : 1) : 2;
    float val = cls == 2 ? res : jd;
    if (active) jd_out[cand] = jd;
    for (int off = 1; off < R; off <<= 1) {
        const int o_cls = __shfl_xor(cls, off), o_r = __shfl_xor(r, off);
        const float o_val = __shfl_xor(val, off);
        const bool take = o_cls < cls || (o_cls == cls && (o_val < val || (o_val == val && o_r < r)));
        cls = take ? o_cls : cls;
        val = take ? o_val : val;
        r = take ? o_r : r;
    }
    if (active && cand - n * R == 0) {
        choice_out[n] = r;
        class_out[n] = cls;
    }
}

static inline bool ch_ik_counts_ok(int N, int R) {
    return N >= 1 && R >= 1 && R <= 64 && (R & (R - 1)) == 0 && (int64_t)N * R <= (int64_t)1 << 30;
}

extern "C" int naf_chain_ik_solve(naf_chain_env_t* h, const float* targets_dev, const float* q_start_dev, const float* seeds_dev, int N,
                                  int R, naf_chain_ik_params_t params, float* q_out, float* residual_out, float* iters_out,
                                  void* stream) {
    if (!h || !targets_dev || !q_start_dev || !seeds_dev || !q_out || !residual_out || !ch_ik_counts_ok(N, R)) return NAF_ERR_ARG;
    if (params.iterations < 1 || !std::isfinite(params.lam2) || !(params.lam2 > 0.f) || !std::isfinite(params.e_max) ||
        !(params.e_max > 0.f) || !std::isfinite(params.dq_max) || !(params.dq_max > 0.f))
        return NAF_ERR_ARG;
    const size_t lds = (size_t)std::max(h->ee_frame, 1) * 6 * 64 * sizeof(float);
    if (lds > CH_MAX_DYN_LDS) return NAF_CHAIN_ERR_LDS;
    // the solve kernels' dynamic LDS (1536 bytes per walked joint) may exceed the 64 KB a kernel gets unasked: both are raised here
    int rc = ch_raise<chain_ik_solve_kernel<false>>();
    if (rc == NAF_OK) rc = ch_raise<chain_ik_solve_kernel<true>>();
    if (rc != NAF_OK) return rc;
    const unsigned grid = (unsigned)(((int64_t)N * R + 63) / 64);
    if (iters_out)
        chain_ik_solve_kernel<true><<<grid, 64, lds, (hipStream_t)stream>>>(h->model_dev, targets_dev, q_start_dev, seeds_dev, N, R, h->A,
                                                                           params, q_out, residual_out, iters_out);
    else
        chain_ik_solve_kernel<false><<<grid, 64, lds, (hipStream_t)stream>>>(h->model_dev, targets_dev, q_start_dev, seeds_dev, N, R, h->A,
                                                                            params, q_out, residual_out, nullptr);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

extern "C" int naf_chain_ik_select(naf_chain_env_t* h, const float* q_out, const float* q_start_dev, const float* residual_out,
                                   const float* probe_dev, const float* cell_dev, int N, int R, float tolerance, float margin,
                                   int* choice_out, int* class_out, float* joint_distance_out, void* stream) {
    if (!h || !q_out || !q_start_dev || !residual_out || !probe_dev || !choice_out || !class_out || !joint_distance_out ||
        !ch_ik_counts_ok(N, R))
        return NAF_ERR_ARG;
    if (!std::isfinite(tolerance) || !(tolerance >= 0.f) || !std::isfinite(margin)) return NAF_ERR_ARG;
    chain_ik_select_kernel<<<(unsigned)(((int64_t)N * R + 63) / 64), 64, 0, (hipStream_t)stream>>>(
        q_out, q_start_dev, residual_out, probe_dev, cell_dev, N, R, h->A, tolerance, margin, choice_out, class_out, joint_distance_out);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

// ---- oriented goal poses: damped least squares on position and end-effector orientation (include/naf_hip.h, "Oriented goal poses")
// chain_ik_solve_kernel's shape — one lane per candidate, a query's R candidates in adjacent lanes, one wave per workgroup, no
// barrier, the same [m][6][lane] LDS record: a_m is already in it, so the angular rows cost no LDS. The walk also returns R_ee.
// Per update pass 1 over LDS accumulates the 21 entries of M = J6 J6^T + lam2 I, the L D L^T factorisation and the two
// substitutions run in registers (every array below is indexed by unrolled loops' compile-time constants only: nothing goes to
// scratch), pass 2 forms dq_m and max |dq_m|. MODE 0: the goal is R_goal, 1: a direction for the tool axis.
#define IK_ORIENT_SMALL 1e-6f
#define IK_PI 3.14159265358979323846f

// index of M's entry (i, j), i <= j, among the 21 of its upper triangle, row by row
__host__ __device__ constexpr int ik_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// the angular error e_w of the end frame's rotation rot[9] against goal (MODE 0: R_goal[9], MODE 1: d[3]): orientation_error's rule
template <int MODE>
__device__ __forceinline__ void ik_orientation_error(const float* rot, const float* goal, const naf_chain_ik_pose_params_t& pp, float* ew) {
    if constexpr (MODE == 1) {
        const float t0 = rot[0] * pp.tool_axis[0] + rot[1] * pp.tool_axis[1] + rot[2] * pp.tool_axis[2];
        const float t1 = rot[3] * pp.tool_axis[0] + rot[4] * pp.tool_axis[1] + rot[5] * pp.tool_axis[2];
        const float t2 = rot[6] * pp.tool_axis[0] + rot[7] * pp.tool_axis[1] + rot[8] * pp.tool_axis[2];
        const float x0 = t1 * goal[2] - t2 * goal[1], x1 = t2 * goal[0] - t0 * goal[2], x2 = t0 * goal[1] - t1 * goal[0];
        const float nx = sqrtf(x0 * x0 + x1 * x1 + x2 * x2);
        const float c = t0 * goal[0] + t1 * goal[1] + t2 * goal[2];
        if (nx <= IK_ORIENT_SMALL) {
            if (c > 0.f) {
                ew[0] = x0; ew[1] = x1; ew[2] = x2;
            } else {      // antiparallel: half a turn about R_ee tool_normal
                ew[0] = IK_PI * (rot[0] * pp.tool_normal[0] + rot[1] * pp.tool_normal[1] + rot[2] * pp.tool_normal[2]);
                ew[1] = IK_PI * (rot[3] * pp.tool_normal[0] + rot[4] * pp.tool_normal[1] + rot[5] * pp.tool_normal[2]);
                ew[2] = IK_PI * (rot[6] * pp.tool_normal[0] + rot[7] * pp.tool_normal[1] + rot[8] * pp.tool_normal[2]);
            }
        } else {
            const float s = atan2f(nx, c) / nx;
            ew[0] = x0 * s; ew[1] = x1 * s; ew[2] = x2 * s;
        }
    } else {
        // E = R_goal R_ee^T
        const float e00 = goal[0] * rot[0] + goal[1] * rot[1] + goal[2] * rot[2];
        const float e01 = goal[0] * rot[3] + goal[1] * rot[4] + goal[2] * rot[5];
        const float e02 = goal[0] * rot[6] + goal[1] * rot[7] + goal[2] * rot[8];
        const float e10 = goal[3] * rot[0] + goal[4] * rot[1] + goal[5] * rot[2];
        const float e11 = goal[3] * rot[3] + goal[4] * rot[4] + goal[5] * rot[5];
        const float e12 = goal[3] * rot[6] + goal[4] * rot[7] + goal[5] * rot[8];
        const float e20 = goal[6] * rot[0] + goal[7] * rot[1] + goal[8] * rot[2];
        const float e21 = goal[6] * rot[3] + goal[7] * rot[4] + goal[8] * rot[5];
        const float e22 = goal[6] * rot[6] + goal[7] * rot[7] + goal[8] * rot[8];
        const float tr = e00 + e11 + e22;
        float x, y, z, w;      // the quaternion of E by the largest-of-four rule, up to a positive factor
        if (tr >= e00 && tr >= e11 && tr >= e22) {
            x = e21 - e12; y = e02 - e20; z = e10 - e01; w = 1.f + tr;
        } else if (e00 >= e11 && e00 >= e22) {
            x = 1.f + e00 - e11 - e22; y = e01 + e10; z = e02 + e20; w = e21 - e12;
        } else if (e11 >= e22) {
            x = e01 + e10; y = 1.f + e11 - e00 - e22; z = e12 + e21; w = e02 - e20;
        } else {
            x = e02 + e20; y = e12 + e21; z = 1.f + e22 - e00 - e11; w = e10 - e01;
        }
        const float len = sqrtf(x * x + y * y + z * z + w * w);
        x /= len; y /= len; z /= len; w /= len;
        if (w < 0.f) {
            x = -x; y = -y; z = -z; w = -w;
        }
        const float nv = sqrtf(x * x + y * y + z * z);
        const float s = nv <= IK_ORIENT_SMALL ? 2.f : 2.f * atan2f(nv, w) / nv;
        ew[0] = x * s; ew[1] = y * s; ew[2] = z * s;
    }
}

// column m of J6 from the joint's LDS record: [a x (ee - p) ; L a] revolute, [a ; 0] prismatic
__device__ __forceinline__ void ik_column6(const float* __restrict__ model, int m, const float* ax, const float* ee, float weight, float* c) {
    const float* w = ax + m * 6 * 64;
    const float a0 = w[0], a1 = w[64], a2 = w[128];
    if (model[CH_HDR + m * CH_JNT + 15] != 0.f) {
        c[0] = a0; c[1] = a1; c[2] = a2;
        c[3] = 0.f; c[4] = 0.f; c[5] = 0.f;
    } else {
        const float d0 = ee[0] - w[192], d1 = ee[1] - w[256], d2 = ee[2] - w[320];
        c[0] = a1 * d2 - a2 * d1;
        c[1] = a2 * d0 - a0 * d2;
        c[2] = a0 * d1 - a1 * d0;
        c[3] = weight * a0; c[4] = weight * a1; c[5] = weight * a2;
    }
}

// M y = e for the symmetric positive definite M (its upper triangle, ik_tri) by L D L^T without pivoting: spd6_solve's eliminations
__device__ __forceinline__ void ik_spd6_solve(const float* M, const float* e, float* y) {
    float l[36], d[6], r[6], z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float v[6];
#pragma unroll
        for (int k = 0; k < j; ++k) v[k] = l[j * 6 + k] * d[k];
        float s = M[ik_tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= l[j * 6 + k] * v[k];
        d[j] = s;
        r[j] = 1.f / s;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float t = M[ik_tri(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= l[i * 6 + k] * v[k];
            l[i * 6 + j] = t * r[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float s = e[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= l[i * 6 + k] * z[k];
        z[i] = s;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        float s = z[i] * r[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= l[k * 6 + i] * y[k];
        y[i] = s;
    }
}

// chain_ik_pose_kernel's update between its walk and ik_update, restated for chain_line_track_kernel below expression for
// expression (calling it from the pose kernel changed that kernel's register allocation and its fused multiply-adds, so the pose
// kernel keeps its own text): from the walk's LDS record, ee and R_ee towards (g0, g1, g2) and the orientation goal it leaves dq_m
// in the record's first float and returns the dq_max scale; ew is the caller's
template <int MODE>
__device__ __forceinline__ float ik_pose_delta(const float* __restrict__ model, int n_joints, float* ax, const float* ee, const float* rot,
                                               float g0, float g1, float g2, const float* goal, const naf_chain_ik_params_t& prm,
                                               const naf_chain_ik_pose_params_t& pp, float* ew) {
    float e[6];
    e[0] = g0 - ee[0]; e[1] = g1 - ee[1]; e[2] = g2 - ee[2];
    const float len = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    if (len > prm.e_max) {
        const float s = prm.e_max / len;
        e[0] *= s; e[1] *= s; e[2] *= s;
    }
    ik_orientation_error<MODE>(rot, goal, pp, ew);
    const float wlen = sqrtf(ew[0] * ew[0] + ew[1] * ew[1] + ew[2] * ew[2]);
    const float ws = wlen > pp.w_max ? pp.w_max / wlen : 1.f;
    e[3] = pp.weight * (ew[0] * ws); e[4] = pp.weight * (ew[1] * ws); e[5] = pp.weight * (ew[2] * ws);
    // pass 1 over LDS: M = sum c c^T + lam2 I, the 21 entries of its upper triangle
    float M[21];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) M[ik_tri(i, j)] = i == j ? prm.lam2 : 0.f;
    for (int m = 0; m < n_joints; ++m) {
        float c[6];
        ik_column6(model, m, ax, ee, pp.weight, c);
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) M[ik_tri(i, j)] += c[i] * c[j];
    }
    float y[6];
    ik_spd6_solve(M, e, y);
    // pass 2: dq_m = c_m . y, kept in the record's first float, and max |dq_m|
    float big = 0.f;
    for (int m = 0; m < n_joints; ++m) {
        float c[6];
        ik_column6(model, m, ax, ee, pp.weight, c);
        const float dq = c[0] * y[0] + c[1] * y[1] + c[2] * y[2] + c[3] * y[3] + c[4] * y[4] + c[5] * y[5];
        ax[m * 6 * 64] = dq;
        big = fmaxf(big, fabsf(dq));
    }
    return big > prm.dq_max ? prm.dq_max / big : 1.f;
}

// MODE 0: goals [N][9] = R_goal, 1: goals [N][3] = d. REC: iters_out as chain_ik_solve_kernel's
template <int MODE, bool REC>
__global__ void __launch_bounds__(64)
chain_ik_pose_kernel(const float* __restrict__ model, const float* __restrict__ targets, const float* __restrict__ goals,
                     const float* __restrict__ q_start, const float* __restrict__ seeds, int N, int R, int A,
                     const naf_chain_ik_params_t prm, const naf_chain_ik_pose_params_t pp, float* q_out,
                     float* __restrict__ residual_out, float* __restrict__ angle_out, float* __restrict__ merit_out,
                     float* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    constexpr int GOAL = MODE == 0 ? 9 : 3;
    const int64_t total = (int64_t)N * R;
    const int64_t cand = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (cand >= total) return;      // (one wave per workgroup and no barrier below)
    const int64_t n = cand / R;
    const int n_joints = (int)model[4];
    float* ax = ch_lds + threadIdx.x;
    float* q = ik_seed<REC>(q_start, seeds, cand, n, R, A, q_out, iters_out);
    const float g0 = targets[n * 3], g1 = targets[n * 3 + 1], g2 = targets[n * 3 + 2];
    float goal[GOAL];
#pragma unroll
    for (int k = 0; k < GOAL; ++k) goal[k] = goals[n * GOAL + k];
    float ee[3], rot[9], ew[3];
    for (int k = 0; k < prm.iterations; ++k) {
        ik_walk<true, true>(model, n_joints, q, ax, ee, rot);
        float e[6];
        e[0] = g0 - ee[0]; e[1] = g1 - ee[1]; e[2] = g2 - ee[2];
        const float len = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        if (len > prm.e_max) {
            const float s = prm.e_max / len;
            e[0] *= s; e[1] *= s; e[2] *= s;
        }
        ik_orientation_error<MODE>(rot, goal, pp, ew);
        const float wlen = sqrtf(ew[0] * ew[0] + ew[1] * ew[1] + ew[2] * ew[2]);
        const float ws = wlen > pp.w_max ? pp.w_max / wlen : 1.f;
        e[3] = pp.weight * (ew[0] * ws); e[4] = pp.weight * (ew[1] * ws); e[5] = pp.weight * (ew[2] * ws);
        // pass 1 over LDS: M = sum c c^T + lam2 I, the 21 entries of its upper triangle
        float M[21];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) M[ik_tri(i, j)] = i == j ? prm.lam2 : 0.f;
        for (int m = 0; m < n_joints; ++m) {
            float c[6];
            ik_column6(model, m, ax, ee, pp.weight, c);
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) M[ik_tri(i, j)] += c[i] * c[j];
        }
        float y[6];
        ik_spd6_solve(M, e, y);
        // pass 2: dq_m = c_m . y, kept in the record's first float, and max |dq_m|
        float big = 0.f;
        for (int m = 0; m < n_joints; ++m) {
            float c[6];
            ik_column6(model, m, ax, ee, pp.weight, c);
            const float dq = c[0] * y[0] + c[1] * y[1] + c[2] * y[2] + c[3] * y[3] + c[4] * y[4] + c[5] * y[5];
            ax[m * 6 * 64] = dq;
            big = fmaxf(big, fabsf(dq));
        }
        const float scale = big > prm.dq_max ? prm.dq_max / big : 1.f;
        ik_update<REC>(model, n_joints, A, scale, ax, q, REC ? iters_out + ((int64_t)(k + 1) * total + cand) * A : nullptr);
    }
    ik_walk<false, true>(model, n_joints, q, ax, ee, rot);
    const float e0 = g0 - ee[0], e1 = g1 - ee[1], e2 = g2 - ee[2];
    const float residual = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    ik_orientation_error<MODE>(rot, goal, pp, ew);
    const float angle = sqrtf(ew[0] * ew[0] + ew[1] * ew[1] + ew[2] * ew[2]);
    residual_out[cand] = residual;
    angle_out[cand] = angle;
    merit_out[cand] = fmaxf(residual, angle * pp.angle_length);
}

template <int MODE, bool REC, typename... Args>
static int ch_ik_pose_launch(unsigned grid, size_t lds, void* stream, Args... args) {
    const int rc = ch_raise<chain_ik_pose_kernel<MODE, REC>>();
    if (rc != NAF_OK) return rc;
    chain_ik_pose_kernel<MODE, REC><<<grid, 64, lds, (hipStream_t)stream>>>(args...);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

extern "C" int naf_chain_ik_solve_pose(naf_chain_env_t* h, const float* targets_dev, const float* goals_dev, int mode,
                                       const float* q_start_dev, const float* seeds_dev, int N, int R, naf_chain_ik_params_t params,
                                       naf_chain_ik_pose_params_t pose_params, float* q_out, float* residual_out, float* angle_out,
                                       float* merit_out, float* iters_out, void* stream) {
    if (!h || !targets_dev || !goals_dev || !q_start_dev || !seeds_dev || !q_out || !residual_out || !angle_out || !merit_out ||
        !ch_ik_counts_ok(N, R) || (mode != 0 && mode != 1))
        return NAF_ERR_ARG;
    const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
    if (params.iterations < 1 || !positive(params.lam2) || !positive(params.e_max) || !positive(params.dq_max) ||
        !positive(pose_params.weight) || !positive(pose_params.w_max) || !positive(pose_params.angle_length))
        return NAF_ERR_ARG;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(pose_params.tool_axis[k]) || !std::isfinite(pose_params.tool_normal[k])) return NAF_ERR_ARG;
    const size_t lds = (size_t)std::max(h->ee_frame, 1) * 6 * 64 * sizeof(float);
    if (lds > CH_MAX_DYN_LDS) return NAF_CHAIN_ERR_LDS;
    const unsigned grid = (unsigned)(((int64_t)N * R + 63) / 64);
    const auto go = [&](auto launch) {
        return launch(grid, lds, stream, h->model_dev, targets_dev, goals_dev, q_start_dev, seeds_dev, N, R, h->A, params, pose_params,
                      q_out, residual_out, angle_out, merit_out, iters_out);
    };
    // the dynamic LDS (1536 bytes per walked joint) may exceed the 64 KB a kernel gets unasked: the launched instantiation is raised
    if (mode == 0)
        return iters_out ? go([](auto... a) { return ch_ik_pose_launch<0, true>(a...); })
                         : go([](auto... a) { return ch_ik_pose_launch<0, false>(a...); });
    return iters_out ? go([](auto... a) { return ch_ik_pose_launch<1, true>(a...); })
                     : go([](auto... a) { return ch_ik_pose_launch<1, false>(a...); });
}

// ---- line moves: the end effector tracks a straight line in the world (include/naf_hip.h, "Line moves") --------------------------
// The two solve kernels' shape — one lane per query, one wave per workgroup, no barrier, the [m][6][lane] LDS record — and their
// updates: ik_pose_delta (MODE 0 full, 1 axis) or ik_delta (MODE 2, position only), then ik_update. The lane's working pose lives
// in its row of nodes_out: row i starts as a copy of row i - 1, takes U updates towards g_i = p0 + (i / W) disp and stays. The
// orientation goal (R_ee, or R_ee tool_axis) and p0 are formed once, from the walk at q_start. Behind a waypoint's updates two more
// walks form its record: one at the node (residual, angle) and one at the middle of the leg that ends there, whose joint values
// ik_walk<.., MID> forms from the two rows as it goes. Trip counts are W and U for every lane. REC: iters_out [W U + 1][N][A].
template <int MODE, bool REC>
__global__ void __launch_bounds__(64)
chain_line_track_kernel(const float* __restrict__ model, const float* __restrict__ q_start, const float* __restrict__ disp, int N, int A,
                        int W, int U, const naf_chain_ik_params_t prm, const naf_chain_ik_pose_params_t pp, float* nodes_out,
                        float* __restrict__ track_out, float* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    constexpr bool ORIENT = MODE != 2;
    constexpr int GOAL = MODE == 0 ? 9 : 3;
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;      // (one wave per workgroup and no barrier below)
    const int n_joints = (int)model[4];
    float* ax = ch_lds + threadIdx.x;
    float* q = nodes_out + n * (W + 1) * A;
    for (int m = 0; m < A; ++m) {
        const float v = q_start[n * A + m];
        q[m] = v;
        if constexpr (REC) iters_out[n * A + m] = v;
    }
    const float d0 = disp[n * 3], d1 = disp[n * 3 + 1], d2 = disp[n * 3 + 2];
    float ee[3], rot[9], ew[3], goal[GOAL];
    ik_walk<false, ORIENT>(model, n_joints, q, ax, ee, rot);
    const float p0 = ee[0], p1 = ee[1], p2 = ee[2];
    if constexpr (MODE == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) goal[k] = rot[k];
    } else if constexpr (MODE == 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            goal[k] = rot[k * 3] * pp.tool_axis[0] + rot[k * 3 + 1] * pp.tool_axis[1] + rot[k * 3 + 2] * pp.tool_axis[2];
    }
    const float fw = (float)W;
    for (int i = 1; i <= W; ++i) {
        const float* prev = q;
        q += A;
        for (int m = 0; m < A; ++m) q[m] = prev[m];
        const float f = (float)i / fw;
        const float g0 = p0 + f * d0, g1 = p1 + f * d1, g2 = p2 + f * d2;
        for (int u = 0; u < U; ++u) {
            float scale;
            if constexpr (ORIENT) {
                ik_walk<true, true>(model, n_joints, q, ax, ee, rot);
                scale = ik_pose_delta<MODE>(model, n_joints, ax, ee, rot, g0, g1, g2, goal, prm, pp, ew);
            } else {
                ik_walk<true>(model, n_joints, q, ax, ee);
                scale = ik_delta(model, n_joints, ax, ee, g0, g1, g2, prm);
            }
            ik_update<REC>(model, n_joints, A, scale, ax, q, REC ? iters_out + (((int64_t)(i - 1) * U + u + 1) * N + n) * A : nullptr);
        }
        // the waypoint's record: residual and angle at the node, the largest joint step, the leg's middle against the line's
        ik_walk<false, ORIENT>(model, n_joints, q, ax, ee, rot);
        const float e0 = g0 - ee[0], e1 = g1 - ee[1], e2 = g2 - ee[2];
        float angle = 0.f;
        if constexpr (ORIENT) {
            ik_orientation_error<MODE>(rot, goal, pp, ew);
            angle = sqrtf(ew[0] * ew[0] + ew[1] * ew[1] + ew[2] * ew[2]);
        }
        float step = 0.f;
        for (int m = 0; m < A; ++m) step = fmaxf(step, fabsf(q[m] - prev[m]));
        ik_walk<false, false, true>(model, n_joints, q, ax, ee, nullptr, prev);
        const float fm = ((float)i - 0.5f) / fw;
        const float h0 = ee[0] - (p0 + fm * d0), h1 = ee[1] - (p1 + fm * d1), h2 = ee[2] - (p2 + fm * d2);
        float* rec = track_out + (n * W + (i - 1)) * NAF_CHAIN_TRACK_FLOATS;
        rec[0] = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
        rec[1] = angle;
        rec[2] = step;
        rec[3] = sqrtf(h0 * h0 + h1 * h1 + h2 * h2);
    }
}

template <int MODE, bool REC, typename... Args>
static int ch_line_track_launch(unsigned grid, size_t lds, void* stream, Args... args) {
    const int rc = ch_raise<chain_line_track_kernel<MODE, REC>>();
    if (rc != NAF_OK) return rc;
    chain_line_track_kernel<MODE, REC><<<grid, 64, lds, (hipStream_t)stream>>>(args...);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

extern "C" int naf_chain_line_track(naf_chain_env_t* h, const float* q_start_dev, const float* disp_dev, int mode, int N, int W, int U,
                                    naf_chain_ik_params_t params, naf_chain_ik_pose_params_t pose_params, float* nodes_out,
                                    float* track_out, float* iters_out, void* stream) {
    if (!h || !q_start_dev || !disp_dev || !nodes_out || !track_out || N < 1 || W < 1 || W > 63 || U < 1 || (int64_t)W * U > 4096 ||
        mode < 0 || mode > 2)
        return NAF_ERR_ARG;
    const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
    if (!positive(params.lam2) || !positive(params.e_max) || !positive(params.dq_max)) return NAF_ERR_ARG;
    if (mode != 2) {
        if (!positive(pose_params.weight) || !positive(pose_params.w_max)) return NAF_ERR_ARG;
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(pose_params.tool_axis[k]) || !std::isfinite(pose_params.tool_normal[k])) return NAF_ERR_ARG;
    }
    const size_t lds = (size_t)std::max(h->ee_frame, 1) * 6 * 64 * sizeof(float);
    if (lds > CH_MAX_DYN_LDS) return NAF_CHAIN_ERR_LDS;
    const unsigned grid = (unsigned)(((int64_t)N + 63) / 64);
    const auto go = [&](auto launch) {
        return launch(grid, lds, stream, h->model_dev, q_start_dev, disp_dev, N, h->A, W, U, params, pose_params, nodes_out, track_out,
                      iters_out);
    };
    // the dynamic LDS (1536 bytes per walked joint) may exceed the 64 KB a kernel gets unasked: the launched instantiation is raised
    if (mode == 0)
        return iters_out ? go([](auto... a) { return ch_line_track_launch<0, true>(a...); })
                         : go([](auto... a) { return ch_line_track_launch<0, false>(a...); });
    if (mode == 1)
        return iters_out ? go([](auto... a) { return ch_line_track_launch<1, true>(a...); })
                         : go([](auto... a) { return ch_line_track_launch<1, false>(a...); });
    return iters_out ? go([](auto... a) { return ch_line_track_launch<2, true>(a...); })
                     : go([](auto... a) { return ch_line_track_launch<2, false>(a...); });
}

// ---- line sweeps: the sampled collision check of a line in joint space (include/naf_hip.h, "Joint paths", "Roadmap edges") -------
// chain_sweep below is the one algorithm; the line is a start -> via -> goal polyline (ViaLine, chain_path_check_kernel) or a
// straight roadmap edge (EdgeLine, chain_edge_check_kernel). One workgroup per line; a lane is one sample of a pass, and the
// workgroup makes S / lanes passes — a trip count the arguments fix. The sample's pose is never stored: the line's end poses are the
// same for the whole workgroup (uniform loads), the lane's fraction is its own, and the walk asks for joint m's value when it
// reaches joint m: one fmaf. So there is no per-lane pose array, no LDS beside the pair phase's end points, nothing in scratch,
// nothing atomic. SC is the probe's shape: wave 0 walks `lanes` samples and stages their capsules' end points as
// [segment][6][lane], every wave joins the pair phase of every pass (its barriers), and only wave 0's lanes keep the running
// minima, the blocked count and the first blocked index; without pairs a workgroup is one wave with no barrier and no LDS. Behind
// the last pass wave 0 reduces them by a butterfly of shuffles and lane 0 writes the record.
//
// A leading ChainCert in the pack (CERT below) is the certifying kernel of naf_chain_path_certify / naf_chain_edge_certify: the
// record has four more floats. Every interval of a leg has the same joint displacement, so how far a point of capsule s can travel
// over half an interval is one number per leg: beta[s] = sum_m |b_m - a_m| reach[m][s] / (2 n) for a leg of n intervals, and for a
// pair (s, t) the same sum over the joints between the two frames with reach[m][t]. Before the first pass the workgroup's threads
// fill the line's tables of n_seg + P such entries in LDS, behind the pair phase's rows — an entry per thread, the joint sum in
// joint order by fmaf, one barrier. A lane picks its table by its sample; the walk and the pair phase subtract the entry from every
// clearance they form and keep those minima beside the plain ones. The kernels without ChainCert keep their arguments.
//
// What the two lines differ in is the Line's, and nothing else is:
//   ViaLine   h = S / 2; sample i is on leg 1 at i / h (i < h) or on leg 2 at (i - h) / (h - 1); three tables — leg 1, leg 2, and
//             their entry-wise maximum for the via sample i == h, which ends one leg's last interval and begins the other's first;
//             the record's floats 5 .. 7 are the two legs' summed length, the larger step, and whether the goal sample is blocked
//   EdgeLine  ONE leg of S - 1 intervals, sample i at i / (S - 1), both ends included; one table, which every sample uses; floats
//             5 .. 7 are the length, the step and 0
//   TrajLine  a law in TIME along a polyline of up to 63 legs (include/naf_hip.h, "Trajectories"): sample i is the tick (float)i dt;
//             one table, of the joints' peak speeds over half a tick; only the samples below the trajectory's own count are LIVE —
//             the others evaluate to the last node and count in nothing (Line::MASKED; absent at compile time for the other two);
//             floats 5 .. 7 are the duration, the largest joint step between two ticks and whether the last live sample is blocked
struct ChainCert {
    const float* reach;      // [A][n_seg] (DEVICE)
    float guard;
};
template <class... Rest>
__device__ static inline const ChainCert& path_cert(const ChainCert& c, const Rest&...) { return c; }
// dynamic LDS of a certifying launch: the SC rows with a second reduction row per wave (none without pairs), then the tables
__host__ __device__ static inline size_t ch_cert_table_floats(int n_seg, int n_pairs, int lanes, int waves) {
    return n_pairs > 0 ? ((size_t)n_seg * 6 + 2 * waves) * lanes : 0;
}
__host__ __device__ static inline size_t ch_cert_lds_bytes(int n_seg, int n_pairs, int lanes, int waves) {
    return (ch_cert_table_floats(n_seg, n_pairs, lanes, waves) + 3 * (size_t)(n_seg + n_pairs)) * sizeof(float);
}

// The line a sweep samples: sample(i) is sample i's fraction (and, for the via line, its leg), pose(sample, m) joint m's value there
// by one fmaf, table_of(i) the sample's table of half-steps, fill(...) entry e of the tables, finish(...) floats 5 .. 7 of the record.
// ViaLine: start -> via over samples 0 .. h, via -> goal over h .. S - 1, h = S / 2; three tables (leg 1, leg 2, their maximum).
struct ViaLine {
    static constexpr bool GOAL = true;      // the record reports whether the last sample, the goal, is blocked
    static constexpr bool MASKED = false;   // every sample counts
    const float *start, *via, *goal;
    int h;
    struct Sample {
        bool second;
        float f;
    };
    __device__ Sample sample(int i) const {
        const bool second = i >= h;
        return {second, second ? (float)(i - h) / (float)(h - 1) : (float)i / (float)h};
    }
    __device__ float pose(const Sample& s, int m) const {
        const float v = via[m];
        const float a = s.second ? v : start[m], b = s.second ? goal[m] : v;
        return fmaf(s.f, b - a, a);
    }
    __device__ int table_of(int i) const { return i < h ? 0 : (i == h ? 2 : 1); }
    __device__ void fill(float* t, int n_tab, int e, int s, int m0, int m1, const float* reach, int n_seg) const {
        float b1 = 0.f, b2 = 0.f;
        for (int m = m0; m < m1; ++m) {
            const float v = via[m], r = reach[m * n_seg + s];
            b1 = fmaf(fabsf(v - start[m]), r, b1);
            b2 = fmaf(fabsf(goal[m] - v), r, b2);
        }
        b1 = b1 / (float)(2 * h);
        b2 = b2 / (float)(2 * (h - 1));
        t[e] = b1;
        t[n_tab + e] = b2;
        t[2 * n_tab + e] = fmaxf(b1, b2);
    }
    __device__ void finish(float* o, int A, int goal_blocked) const {
        float l1 = 0.f, l2 = 0.f;
        for (int m = 0; m < A; ++m) {
            l1 = fmaxf(l1, fabsf(via[m] - start[m]));
            l2 = fmaxf(l2, fabsf(goal[m] - via[m]));
        }
        o[5] = l1 + l2;
        o[6] = fmaxf(l1 / (float)h, l2 / (float)(h - 1));
        o[7] = (float)goal_blocked;
    }
};
// EdgeLine: a -> b over samples 0 .. S - 1, both ends included; ONE table, and fill writes nothing beyond t[e]: an edge launch
// has LDS for one.
struct EdgeLine {
    static constexpr bool GOAL = false;
    static constexpr bool MASKED = false;
    const float *a, *b;
    int last;      // S - 1
    __device__ float sample(int i) const { return (float)i / (float)last; }
    __device__ float pose(float f, int m) const {
        const float lo = a[m];
        return fmaf(f, b[m] - lo, lo);
    }
    __device__ int table_of(int) const { return 0; }
    __device__ void fill(float* t, int, int e, int s, int m0, int m1, const float* reach, int n_seg) const {
        float acc = 0.f;
        for (int m = m0; m < m1; ++m) acc = fmaf(fabsf(b[m] - a[m]), reach[m * n_seg + s], acc);
        t[e] = acc / (float)(2 * last);
    }
    __device__ void finish(float* o, int A, int) const {
        float len = 0.f;
        for (int m = 0; m < A; ++m) len = fmaxf(len, fabsf(b[m] - a[m]));
        o[5] = len;
        o[6] = len / (float)last;
        o[7] = 0.f;
    }
};

// TrajLine: linear segments with parabolic blends in time (environment/trajectory.py states the law). The schedule is the host's:
// nodes P_k, and per node (t_k, tau_k, 1 / T_k). sample(i) finds the leg j of t = (float)i dt — how many node times are <= t, a
// uniform scan of at most 64 — and what of the law does not depend on the joint; pose(sample, m) forms the three velocities it
// needs from four node values. Legs 0 and K + 1 are the virtual ones: their 1 / T reads as 0 and their node indices are clamped,
// so v_0 = v_{K+1} = 0 without a branch. Nothing but the node loads is indexed per lane.
struct TrajLine {
    static constexpr bool GOAL = true;      // float 7: whether the last LIVE sample is blocked
    static constexpr bool MASKED = true;    // samples i >= live count in nothing
    const float *nodes, *times, *vpeak;     // [V][A], [V][3], [A] of this trajectory
    int A, n, live;                         // n = K + 1 nodes; live = S_n
    float dt;
    struct Sample {
        int j;
        float s, c0, c1, wm, w, wp;         // c0 = h0^2 / (2 tau_{j-1}), c1 = h1^2 / (2 tau_j); 1 / T of legs j - 1, j, j + 1 (0: virtual)
    };
    __device__ Sample sample(int i) const {
        const float t = (float)i * dt;
        int j = 0;
        for (int k = 0; k < n; ++k) j += times[3 * k] <= t ? 1 : 0;
        const int K = n - 1;
        const int jp = max(j - 1, 0), jn = min(j, K), jq = min(j + 1, K);
        const float s = t - (j >= 1 ? times[3 * jp] : 0.f);
        const float tau_p = j >= 1 ? times[3 * jp + 1] : 0.f, tau_n = j <= K ? times[3 * jn + 1] : 0.f;
        const float h0 = fmaxf(0.f, 0.5f * tau_p - s);
        const float h1 = j <= K ? fmaxf(0.f, (t - times[3 * jn]) + 0.5f * tau_n) : 0.f;
        const float c0 = tau_p > 0.f ? 0.5f * h0 * h0 * (1.f / tau_p) : 0.f, c1 = tau_n > 0.f ? 0.5f * h1 * h1 * (1.f / tau_n) : 0.f;
        return {j, s, c0, c1, j >= 2 ? times[3 * jp + 2] : 0.f, j >= 1 && j <= K ? times[3 * jn + 2] : 0.f,
                j + 1 <= K ? times[3 * jq + 2] : 0.f};
    }
    __device__ float pose(const Sample& at, int m) const {
        const int K = n - 1;
        const float pm2 = nodes[max(at.j - 2, 0) * A + m], pm1 = nodes[max(at.j - 1, 0) * A + m];
        const float p0 = nodes[min(at.j, K) * A + m], p1 = nodes[min(at.j + 1, K) * A + m];
        const float v_prev = (pm1 - pm2) * at.wm, v = (p0 - pm1) * at.w, v_next = (p1 - p0) * at.wp;
        return fmaf(at.c1, v_next - v, fmaf(at.c0, v - v_prev, fmaf(v, at.s, pm1)));
    }
    __device__ bool counts(int i) const { return i < live; }
    __device__ int last() const { return live - 1; }
    __device__ int table_of(int) const { return 0; }
    __device__ void fill(float* t, int, int e, int s, int m0, int m1, const float* reach, int n_seg) const {
        float acc = 0.f;
        for (int m = m0; m < m1; ++m) acc = fmaf(vpeak[m], reach[m * n_seg + s], acc);
        t[e] = (0.5f * dt) * acc;
    }
    __device__ void finish(float* o, int, int last_blocked) const {
        float step = 0.f;
        for (int m = 0; m < A; ++m) step = fmaxf(step, vpeak[m] * dt);
        o[5] = times[3 * (n - 1)] + 0.5f * times[3 * (n - 1) + 1];
        o[6] = step;
        o[7] = (float)last_blocked;
    }
};

// The sweep of workgroup `item` along `line`: `record` is the item's own, poses_out (or nullptr) the launch's [item][S][A].
template <bool SC, class Line, class... Cell>
__device__ __forceinline__ void chain_sweep(const float* __restrict__ model, const Line& line, float ox, float oy, float oz, float orad,
                                            int S, int A, int n_seg, int n_pairs, int lanes, float margin, float* __restrict__ record,
                                            float* __restrict__ poses_out, int64_t item, const Cell&... cell) {
    constexpr bool CELL = (std::is_same_v<Cell, ChainCell> || ... || false);
    constexpr bool BOX = (std::is_same_v<Cell, ChainBox> || ... || false);
    constexpr bool CERT = (std::is_same_v<Cell, ChainCert> || ... || false);
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    const int lane = threadIdx.x & 63;
    const bool active = lane < lanes;
    const bool walker = active && threadIdx.x < 64;
    float min_clear = INFINITY, min_self = INFINITY, min_cell = INFINITY;
    int first = INT_MAX, count = 0, goal_blocked = 0;
    float low_clear = INFINITY, low_self = INFINITY, low_cell = INFINITY, guard = 0.f;
    int first_low = INT_MAX;
    const int n_tab = n_seg + n_pairs;
    const float* tab = nullptr;
    if constexpr (CERT) {
        const ChainCert& cert = path_cert(cell...);
        const float* segs = model + ch_off_seg(A);
        const float* pairs = model + ch_off_pair(A, n_seg);
        float* t = ch_lds + ch_cert_table_floats(n_seg, n_pairs, lanes, blockDim.x >> 6);
        for (int e = threadIdx.x; e < n_tab; e += blockDim.x) {
            // entry e < n_seg: segment e against the world, joints 0 .. frame - 1; else pair (s, t): t against s, joints frame s ..
            const int s = e < n_seg ? e : (int)pairs[2 * (e - n_seg) + 1];
            const int m0 = e < n_seg ? 0 : (int)segs[(int)pairs[2 * (e - n_seg)] * CH_SEG];
            const int m1 = (int)segs[s * CH_SEG];
            line.fill(t, n_tab, e, s, m0, m1, cert.reach, n_seg);
        }
        __syncthreads();
        tab = t;
        guard = cert.guard;
    }
    for (int base = 0; base < S; base += lanes) {      // (uniform: every thread takes every pass)
        const int i = base + lane;
        const auto at = line.sample(i);
        float ee[3];
        WalkAux aux = {SC ? ch_lds + lane : nullptr, lanes, INFINITY, INFINITY, CERT ? tab + line.table_of(i) * n_tab : nullptr,
                       INFINITY, INFINITY};
        if (walker) {
            float* rec = poses_out ? poses_out + (item * S + i) * A : nullptr;
            chain_walk_at<SC, true, false, true, CELL, BOX, CERT>(
                model, A, n_seg,
                [=](int m) {
                    const float q = line.pose(at, m);
                    if (rec) rec[m] = q;
                    return q;
                },
                ox, oy, oz, orad, nullptr, nullptr, ee, aux);
        }
        float self_clear = INFINITY, self_slack = INFINITY;
        if constexpr (SC)
            self_clear = self_clearance_phase<CERT>(model, A, n_seg, n_pairs, ch_lds, lanes, lane, active,
                                                    CERT ? aux.beta + n_seg : nullptr, &self_slack);
        if (walker) {
            if constexpr (Line::MASKED)      // (a dead sample walked, wrote its pose, and counts in nothing; this ends the pass's body)
                if (!line.counts(i)) continue;
            const float clear = aux.clear - orad;
            const bool blocked = clear < margin || self_clear < margin || (CELL && aux.cell < margin);
            min_clear = fminf(min_clear, clear);
            min_self = fminf(min_self, self_clear);
            if constexpr (CELL) min_cell = fminf(min_cell, aux.cell);
            first = blocked && i < first ? i : first;
            count += blocked ? 1 : 0;
            if constexpr (Line::MASKED) goal_blocked |= blocked && i == line.last() ? 1 : 0;
            else if constexpr (Line::GOAL) goal_blocked |= blocked && i == S - 1 ? 1 : 0;
            if constexpr (CERT) {
                const float s0 = aux.slack - orad - guard, s1 = self_slack - guard, s2 = aux.cell_slack - guard;
                low_clear = fminf(low_clear, s0);
                low_self = fminf(low_self, s1);
                if constexpr (CELL) low_cell = fminf(low_cell, s2);
                first_low = (s0 < margin || s1 < margin || (CELL && s2 < margin)) && i < first_low ? i : first_low;
            }
        }
    }
    if (threadIdx.x >= 64) return;      // (behind the last barrier; wave 0 is whole: the lanes that walked nothing hold the identities)
    for (int off = 32; off > 0; off >>= 1) {
        min_clear = fminf(min_clear, __shfl_xor(min_clear, off));
        min_self = fminf(min_self, __shfl_xor(min_self, off));
        min_cell = fminf(min_cell, __shfl_xor(min_cell, off));
        first = min(first, __shfl_xor(first, off));
        count += __shfl_xor(count, off);
        if constexpr (Line::GOAL) goal_blocked |= __shfl_xor(goal_blocked, off);
        if constexpr (CERT) {
            low_clear = fminf(low_clear, __shfl_xor(low_clear, off));
            low_self = fminf(low_self, __shfl_xor(low_self, off));
            low_cell = fminf(low_cell, __shfl_xor(low_cell, off));
            first_low = min(first_low, __shfl_xor(first_low, off));
        }
    }
    if (threadIdx.x != 0) return;
    record[0] = min_clear;
    record[1] = min_self;
    record[2] = min_cell;
    record[3] = first == INT_MAX ? -1.f : (float)first;
    record[4] = (float)count;
    line.finish(record, A, goal_blocked);
    if constexpr (CERT) {
        record[8] = low_clear;
        record[9] = low_self;
        record[10] = low_cell;
        record[11] = first_low == INT_MAX ? -1.f : (float)first_low;
    }
}

// one workgroup per candidate path (query n, via c)
template <bool SC, class... Cell>
__global__ void __launch_bounds__(SC ? 64 * CH_MAX_WAVES : 64)
chain_path_check_kernel(const float* __restrict__ model, const float* __restrict__ q_start, const float* __restrict__ q_goal,
                        const float* __restrict__ vias, const float* __restrict__ obstacles, float orad, int C, int S, int A, int n_seg,
                        int n_pairs, int lanes, float margin, float* __restrict__ out, float* __restrict__ poses_out, const Cell... cell) {
    constexpr bool CERT = (std::is_same_v<Cell, ChainCert> || ... || false);
    const int64_t cand = blockIdx.x;
    const int64_t n = cand / C;
    const ViaLine line = {q_start + n * A, vias + cand * A, q_goal + n * A, S >> 1};
    chain_sweep<SC>(model, line, obstacles[n * 3], obstacles[n * 3 + 1], obstacles[n * 3 + 2], orad, S, A, n_seg, n_pairs, lanes, margin,
                    out + cand * (CERT ? NAF_CHAIN_PATH_CERT_FLOATS : NAF_CHAIN_PATH_FLOATS),
                    poses_out, cand, cell...);
}

// what naf_chain_path_check and naf_chain_path_certify ask of the arguments they share
static inline bool ch_path_args_ok(int N, int C, int S, float margin, float obstacle_radius) {
    if (N < 1 || C < 1 || C > 64 || S < 64 || S > 2048 || S % 64 != 0 || (int64_t)N * C > (int64_t)1 << 30) return false;
    return std::isfinite(margin) && std::isfinite(obstacle_radius) && obstacle_radius >= 0.f;
}

// The SC path kernels' dynamic LDS is the probe's. One workgroup per candidate path.
extern "C" int naf_chain_path_check(naf_chain_env_t* h, const float* q_start_dev, const float* q_goal_dev, const float* vias_dev,
                                    const float* obstacles_dev, float obstacle_radius, int N, int C, int S, float margin, float* out,
                                    float* poses_out, void* stream) {
    if (!h || !q_start_dev || !q_goal_dev || !vias_dev || !obstacles_dev || !out) return NAF_ERR_ARG;
    if (!ch_path_args_ok(N, C, S, margin, obstacle_radius)) return NAF_ERR_ARG;
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        const ChShape w = ch_shape<sc()>(h, h->waves);
        return ch_launch_raising<chain_path_check_kernel<sc(), decltype(cell)...>>(
            CH_MAX_DYN_LDS, (unsigned)((int64_t)N * C), w, stream, h->model_dev, q_start_dev, q_goal_dev, vias_dev, obstacles_dev,
            obstacle_radius, C, S, h->A, h->n_seg, w.n_pairs, w.lanes, margin, out, poses_out, cell...);
    });
}

extern "C" int naf_chain_path_certify(naf_chain_env_t* h, const float* q_start_dev, const float* q_goal_dev, const float* vias_dev,
                                      const float* obstacles_dev, float obstacle_radius, const float* reach_dev, float guard, int N,
                                      int C, int S, float margin, float* out, float* poses_out, void* stream) {
    if (!h || !q_start_dev || !q_goal_dev || !vias_dev || !obstacles_dev || !reach_dev || !out) return NAF_ERR_ARG;
    if (!ch_path_args_ok(N, C, S, margin, obstacle_radius)) return NAF_ERR_ARG;
    if (!std::isfinite(guard) || guard < 0.f) return NAF_ERR_ARG;
    // the tables and the second reduction row on top of the handle's rows: an arm they do not fit with is refused, not shrunk
    const size_t lds = ch_cert_lds_bytes(h->n_seg, h->n_pairs, h->lanes, h->waves);
    if (lds > (h->n_pairs > 0 ? CH_MAX_DYN_LDS : 64 * 1024)) return NAF_CHAIN_ERR_LDS;
    const ChainCert cert = {reach_dev, guard};
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        ChShape w = ch_shape<sc()>(h, h->waves);
        w.lds = lds;      // (the tables: also without pairs)
        return ch_launch_raising<chain_path_check_kernel<sc(), ChainCert, decltype(cell)...>>(
            CH_MAX_DYN_LDS, (unsigned)((int64_t)N * C), w, stream, h->model_dev, q_start_dev, q_goal_dev, vias_dev, obstacles_dev,
            obstacle_radius, C, S, h->A, h->n_seg, w.n_pairs, w.lanes, margin, out, poses_out, cert, cell...);
    });
}

// ---- roadmap edges: the sampled collision check of straight joint-space edges (include/naf_hip.h, "Roadmap edges") ---------------
// chain_sweep along an EdgeLine. One workgroup per (query n, edge e); the edge's two nodes are read from edges[e] (the same list
// for every query of the launch) and their poses from nodes[n] — uniform loads. A leading ChainCert in the pack is
// naf_chain_edge_certify's kernel: the record has NAF_CHAIN_EDGE_CERT_FLOATS floats.
template <bool SC, class... Cell>
__global__ void __launch_bounds__(SC ? 64 * CH_MAX_WAVES : 64)
chain_edge_check_kernel(const float* __restrict__ model, const float* __restrict__ nodes, const int32_t* __restrict__ edges,
                        const float* __restrict__ obstacles, float orad, int V, int E, int S, int A, int n_seg, int n_pairs, int lanes,
                        float margin, float* __restrict__ out, float* __restrict__ poses_out, const Cell... cell) {
    constexpr bool CERT = (std::is_same_v<Cell, ChainCert> || ... || false);
    const int64_t item = blockIdx.x;
    const int64_t n = item / E;
    const int e = (int)(item - n * E);
    // (the host validated 0 <= i < j < V for every edge before the upload; the clamp keeps a stray index inside the query's nodes)
    const int ni = min(max(edges[2 * e], 0), V - 1), nj = min(max(edges[2 * e + 1], 0), V - 1);
    const EdgeLine line = {nodes + (n * V + ni) * A, nodes + (n * V + nj) * A, S - 1};
    chain_sweep<SC>(model, line, obstacles[n * 3], obstacles[n * 3 + 1], obstacles[n * 3 + 2], orad, S, A, n_seg, n_pairs, lanes, margin,
                    out + item * (CERT ? NAF_CHAIN_EDGE_CERT_FLOATS : NAF_CHAIN_EDGE_FLOATS),
                    poses_out, item, cell...);
}

// what naf_chain_edge_check and naf_chain_edge_certify ask of the arguments they share
static inline bool ch_edge_args_ok(int N, int V, int E, int S, float margin, float obstacle_radius) {
    if (N < 1 || V < 2 || V > 64 || E < 1 || E > V * (V - 1) / 2 || (int64_t)N * E > (int64_t)1 << 30) return false;
    if (S < 64 || S > 2048 || S % 64 != 0) return false;
    return std::isfinite(margin) && std::isfinite(obstacle_radius) && obstacle_radius >= 0.f;
}

// One workgroup per (query, edge); the SC kernels' dynamic LDS is the probe's.
extern "C" int naf_chain_edge_check(naf_chain_env_t* h, const float* nodes_dev, const int32_t* edges_dev, const float* obstacles_dev,
                                    float obstacle_radius, int N, int V, int E, int S, float margin, float* out, float* poses_out,
                                    void* stream) {
    if (!h || !nodes_dev || !edges_dev || !obstacles_dev || !out) return NAF_ERR_ARG;
    if (!ch_edge_args_ok(N, V, E, S, margin, obstacle_radius)) return NAF_ERR_ARG;
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        const ChShape w = ch_shape<sc()>(h, h->waves);
        return ch_launch_raising<chain_edge_check_kernel<sc(), decltype(cell)...>>(
            CH_MAX_DYN_LDS, (unsigned)((int64_t)N * E), w, stream, h->model_dev, nodes_dev, edges_dev, obstacles_dev, obstacle_radius,
            V, E, S, h->A, h->n_seg, w.n_pairs, w.lanes, margin, out, poses_out, cell...);
    });
}

// The certifying edge launch: the SC rows with the second reduction row per wave (none without pairs), then the edge's one table.
extern "C" int naf_chain_edge_certify(naf_chain_env_t* h, const float* nodes_dev, const int32_t* edges_dev, const float* obstacles_dev,
                                      float obstacle_radius, const float* reach_dev, float guard, int N, int V, int E, int S,
                                      float margin, float* out, float* poses_out, void* stream) {
    if (!h || !nodes_dev || !edges_dev || !obstacles_dev || !reach_dev || !out) return NAF_ERR_ARG;
    if (!ch_edge_args_ok(N, V, E, S, margin, obstacle_radius)) return NAF_ERR_ARG;
    if (!std::isfinite(guard) || guard < 0.f) return NAF_ERR_ARG;
    // an arm whose rows do not leave room for the table and the second row is refused, not shrunk: naf_chain_path_certify's rule
    const size_t lds = (ch_cert_table_floats(h->n_seg, h->n_pairs, h->lanes, h->waves) + (size_t)(h->n_seg + h->n_pairs)) * sizeof(float);
    if (lds > (h->n_pairs > 0 ? CH_MAX_DYN_LDS : 64 * 1024)) return NAF_CHAIN_ERR_LDS;
    const ChainCert cert = {reach_dev, guard};
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        ChShape w = ch_shape<sc()>(h, h->waves);
        w.lds = lds;      // (the table: also without pairs)
        return ch_launch_raising<chain_edge_check_kernel<sc(), ChainCert, decltype(cell)...>>(
            CH_MAX_DYN_LDS, (unsigned)((int64_t)N * E), w, stream, h->model_dev, nodes_dev, edges_dev, obstacles_dev, obstacle_radius,
            V, E, S, h->A, h->n_seg, w.n_pairs, w.lanes, margin, out, poses_out, cert, cell...);
    });
}

// ---- trajectories: a time law along a polyline, checked at a controller's ticks (include/naf_hip.h, "Trajectories") --------------
// chain_sweep along a TrajLine. One workgroup per trajectory n: its nodes, times, peak speeds and counts are uniform loads. A leading
// ChainCert in the pack is naf_chain_traj_certify's kernel: the record has NAF_CHAIN_EDGE_CERT_FLOATS floats.
template <bool SC, class... Cell>
__global__ void __launch_bounds__(SC ? 64 * CH_MAX_WAVES : 64)
chain_traj_check_kernel(const float* __restrict__ model, const float* __restrict__ nodes, const int32_t* __restrict__ n_nodes,
                        const float* __restrict__ times, const float* __restrict__ vpeak, const int32_t* __restrict__ n_samples,
                        const float* __restrict__ obstacles, float orad, float dt, int V, int S, int A, int n_seg, int n_pairs,
                        int lanes, float margin, float* __restrict__ out, float* __restrict__ poses_out, const Cell... cell) {
    constexpr bool CERT = (std::is_same_v<Cell, ChainCert> || ... || false);
    const int64_t n = blockIdx.x;
    // (the host validated 1 <= n_nodes <= V and 1 <= n_samples <= S before the upload; the clamps keep a stray count inside)
    const TrajLine line = {nodes + n * V * A, times + n * V * 3, vpeak + n * A, A, min(max(n_nodes[n], 1), V),
                           min(max(n_samples[n], 1), S), dt};
    chain_sweep<SC>(model, line, obstacles[n * 3], obstacles[n * 3 + 1], obstacles[n * 3 + 2], orad, S, A, n_seg, n_pairs, lanes, margin,
                    out + n * (CERT ? NAF_CHAIN_EDGE_CERT_FLOATS : NAF_CHAIN_EDGE_FLOATS), poses_out, n, cell...);
}

// what naf_chain_traj_check and naf_chain_traj_certify ask of the arguments they share
static inline bool ch_traj_args_ok(int N, int V, int S, float dt, float margin, float obstacle_radius) {
    if (N < 1 || N > 1 << 30 || V < 2 || V > 64 || S < 64 || S > 8192 || S % 64 != 0) return false;
    return std::isfinite(dt) && dt > 0.f && std::isfinite(margin) && std::isfinite(obstacle_radius) && obstacle_radius >= 0.f;
}

// One workgroup per trajectory; the SC kernels' dynamic LDS is the probe's.
extern "C" int naf_chain_traj_check(naf_chain_env_t* h, const float* nodes_dev, const int32_t* n_nodes_dev, const float* times_dev,
                                    const float* vpeak_dev, const int32_t* n_samples_dev, const float* obstacles_dev,
                                    float obstacle_radius, float dt, int N, int V, int S, float margin, float* out, float* poses_out,
                                    void* stream) {
    if (!h || !nodes_dev || !n_nodes_dev || !times_dev || !vpeak_dev || !n_samples_dev || !obstacles_dev || !out) return NAF_ERR_ARG;
    if (!ch_traj_args_ok(N, V, S, dt, margin, obstacle_radius)) return NAF_ERR_ARG;
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        const ChShape w = ch_shape<sc()>(h, h->waves);
        return ch_launch_raising<chain_traj_check_kernel<sc(), decltype(cell)...>>(
            CH_MAX_DYN_LDS, (unsigned)N, w, stream, h->model_dev, nodes_dev, n_nodes_dev, times_dev, vpeak_dev, n_samples_dev,
            obstacles_dev, obstacle_radius, dt, V, S, h->A, h->n_seg, w.n_pairs, w.lanes, margin, out, poses_out, cell...);
    });
}

// The certifying trajectory launch: naf_chain_edge_certify's LDS — the SC rows with the second reduction row per wave, then ONE table.
extern "C" int naf_chain_traj_certify(naf_chain_env_t* h, const float* nodes_dev, const int32_t* n_nodes_dev, const float* times_dev,
                                      const float* vpeak_dev, const int32_t* n_samples_dev, const float* obstacles_dev,
                                      float obstacle_radius, const float* reach_dev, float guard, float dt, int N, int V, int S,
                                      float margin, float* out, float* poses_out, void* stream) {
    if (!h || !nodes_dev || !n_nodes_dev || !times_dev || !vpeak_dev || !n_samples_dev || !obstacles_dev || !reach_dev || !out)
        return NAF_ERR_ARG;
    if (!ch_traj_args_ok(N, V, S, dt, margin, obstacle_radius)) return NAF_ERR_ARG;
    if (!std::isfinite(guard) || guard < 0.f) return NAF_ERR_ARG;
    const size_t lds = (ch_cert_table_floats(h->n_seg, h->n_pairs, h->lanes, h->waves) + (size_t)(h->n_seg + h->n_pairs)) * sizeof(float);
    if (lds > (h->n_pairs > 0 ? CH_MAX_DYN_LDS : 64 * 1024)) return NAF_CHAIN_ERR_LDS;
    const ChainCert cert = {reach_dev, guard};
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        ChShape w = ch_shape<sc()>(h, h->waves);
        w.lds = lds;      // (the table: also without pairs)
        return ch_launch_raising<chain_traj_check_kernel<sc(), ChainCert, decltype(cell)...>>(
            CH_MAX_DYN_LDS, (unsigned)N, w, stream, h->model_dev, nodes_dev, n_nodes_dev, times_dev, vpeak_dev, n_samples_dev,
            obstacles_dev, obstacle_radius, dt, V, S, h->A, h->n_seg, w.n_pairs, w.lanes, margin, out, poses_out, cert, cell...);
    });
}

// ---- demonstrations: planned joint paths as replay rows (include/naf_hip.h, "Demonstrations") -------------------------------------
// One workgroup per demonstration; a lane is one POSE of a pass: lane t walks p_t once with the walk that writes an observation,
// straight into row t's `state`, copies it into row t - 1's `next_state` and writes row t - 1's action, reward, done and zero tail
// from the outcome of that walk. A row is thus filled by two lanes with disjoint floats, and nothing is atomic. The poses follow the
// step kernel's recurrence, not a closed form: the pass's base pose (and the velocities the step before it reported) lies in LDS
// laid out as env_state is — pose[A] | target | obstacle | velocity[A] — so that the walk reads the scene from it as it does from
// env_state; the walk's accessor advances joint m from the base by one fused step per tick up to the lane's own tick (at most
// `lanes` trips), and behind the pass wave 0 advances the base by `lanes` ticks, a joint per lane. No per-lane pose array, nothing in
// scratch. Only wave 0 ever touches the base, in program order, so it needs no barrier: demo_wave_order keeps the compiler from
// moving the accesses across it. SC is the path kernel's shape: every wave joins the pair phase of every pass.
__device__ static inline void demo_tick(const float* j, float a, float& q, float& vel) {
    q = fmaf(CH_DT, a, q);      // the step kernels' `st[m] + CH_DT * a`, which the compiler contracts to this one operation in each
    vel = a;
    if (j[16] != 0.f) {
        if (q > j[18]) { q = j[18]; vel = 0.f; }
        if (q < j[17]) { q = j[17]; vel = 0.f; }
    }
}

__device__ static inline void demo_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__host__ __device__ static inline int ch_demo_base_floats(int A) { return 2 * A + 6; }

template <bool SC, class... Cell>
__global__ void __launch_bounds__(SC ? 64 * CH_MAX_WAVES : 64)
chain_demo_rows_kernel(const float* __restrict__ model, const float* __restrict__ q_start, const float* __restrict__ leg_actions,
                       const int* __restrict__ n_ticks, const float* __restrict__ targets, const float* __restrict__ obstacles,
                       float orad, int T_cap, int A, int n_seg, int n_pairs, int lanes, int row_floats, float* __restrict__ rows_out,
                       float* __restrict__ records_out, float* __restrict__ poses_out, const Cell... cell) {
    constexpr bool CELL = (std::is_same_v<Cell, ChainCell> || ... || false);
    constexpr bool BOX = (std::is_same_v<Cell, ChainBox> || ... || false);
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    const int64_t n = blockIdx.x;
    const int S = 2 * A + 9;
    const int off_s2 = naf_row_off_s2(S, A), off_d = naf_row_off_done(S, A);
    // (the host validated the counts; the clamps only keep a wrong upload inside the arrays)
    const int n1 = min(max(n_ticks[2 * n], 1), 1 << 20), n12 = n1 + min(max(n_ticks[2 * n + 1], 1), 1 << 20);
    const int T = min(n12, T_cap);                       // rows of this demonstration; poses 0 .. T
    const float* a1 = leg_actions + n * 2 * A;
    const float* a2 = a1 + A;
    const float ox = obstacles[n * 3], oy = obstacles[n * 3 + 1], oz = obstacles[n * 3 + 2];
    const float tx = targets[n * 3], ty = targets[n * 3 + 1], tz = targets[n * 3 + 2];
    const int lane = threadIdx.x & 63;
    const bool active = lane < lanes;
    const bool wave0 = threadIdx.x < 64;
    float* base = ch_lds + (SC ? ch_lds_bytes(n_seg, lanes, blockDim.x >> 6) / sizeof(float) : 0);
    float* rows = rows_out + n * T_cap * row_floats;
    if (wave0) {
        for (int m = lane; m < A; m += 64) {
            const float* j = model + CH_HDR + m * CH_JNT;
            float q = q_start[n * A + m];
            if (j[16] != 0.f) {      // p_0: the start pose clamped into the limits, as naf_chain_env_reset_given clamps it
                if (q > j[18]) q = j[18];
                if (q < j[17]) q = j[17];
            }
            base[m] = q;
            base[A + 6 + m] = 0.f;
        }
        if (lane < 3) {
            base[A + lane] = targets[n * 3 + lane];
            base[A + 3 + lane] = obstacles[n * 3 + lane];
        }
        demo_wave_order();
    }
    float min_clear = INFINITY, min_self = INFINITY, min_cell = INFINITY, final_dist = -1.f;
    int first_key = INT_MAX;      // 8 x (row of the first done) + its end code
    bool stopped = false;         // (uniform in wave 0) a pass before this one held the first done
    for (int b = 0; b <= T; b += lanes) {      // (uniform: every thread takes every pass)
        const int t = b + lane;
        const bool walks = active && wave0 && t <= T;
        float* prev = rows + (int64_t)(t - 1) * row_floats;      // row t - 1: used only where t >= 1
        float* o = t < T ? prev + row_floats : prev + off_s2;    // obs(p_t): row t's state, or the last row's next_state
        float ee[3];
        bool hit = false;
        WalkAux aux = {SC ? ch_lds + lane : nullptr, lanes, INFINITY, INFINITY};
        if (walks) {
            float* rec = poses_out ? poses_out + ((n * (T_cap + 1)) + t) * A : nullptr;
            hit = chain_walk_at<SC, false, false, true, CELL, BOX>(
                model, A, n_seg,
                [=](int m) {
                    const float* j = model + CH_HDR + m * CH_JNT;
                    const float u = a1[m], v = a2[m];
                    float q = base[m], vel = base[A + 6 + m];
                    for (int k = b; k < t; ++k) demo_tick(j, k < n1 ? u : v, q, vel);
                    const int slot = (int)j[21];
                    if (slot >= 0) o[A + slot] = vel;      // what step t - 1 reported (0 at t = 0, 0 where a limit stopped the joint)
                    if (rec) rec[m] = q;
                    return q;
                },
                ox, oy, oz, orad, base, o, ee, aux);
        }
        float self_clear = INFINITY;
        if constexpr (SC) self_clear = self_clearance_phase(model, A, n_seg, n_pairs, ch_lds, lanes, lane, active && t <= T);
        if (wave0) {
            const bool outcome = walks && t >= 1;      // the walk of p_t is the outcome of row t - 1
            float dist = 0.f, clear = INFINITY, cellc = INFINITY;
            bool done = false;
            int code = 0;
            if (outcome) {
                const float dx = ee[0] - tx, dy = ee[1] - ty, dz = ee[2] - tz;
                dist = sqrtf(dx * dx + dy * dy + dz * dz);
                clear = aux.clear - orad;
                if constexpr (CELL) cellc = aux.cell;
                const bool reached = dist < CH_REACHED, self_hit = self_clear < 0.f, cell_hit = CELL && aux.cell < 0.f;
                const bool any = hit || self_hit || cell_hit;
                done = reached || any;
                code = reached ? 1 : (hit ? 2 : (self_hit ? 3 : (cell_hit ? 4 : 0)));
                const float* act = t - 1 < n1 ? a1 : a2;
                for (int m = 0; m < A; ++m) prev[S + m] = act[m];
                prev[S + A] = reached ? 250.f : (any ? -1000.f : -(dist - CH_REACHED));
                for (int k = S + A + 1; k < off_s2; ++k) prev[k] = 0.f;
                if (t < T)
                    for (int k = 0; k < S; ++k) prev[off_s2 + k] = o[k];
                prev[off_d] = done ? 1.f : 0.f;
                for (int k = off_d + 1; k < row_floats; ++k) prev[k] = 0.f;      // the tag float included: an untagged row
            }
            const unsigned long long mask = __ballot(outcome && done);
            const int first_lane = mask ? __ffsll(mask) - 1 : 64;
            if (!stopped && outcome && lane <= first_lane) {      // rows up to the first done are the demonstration's
                min_clear = fminf(min_clear, clear);
                min_self = fminf(min_self, self_clear);
                min_cell = fminf(min_cell, cellc);
                if (lane == first_lane) { first_key = (t - 1) * 8 + code; final_dist = dist; }
                else if (t == T && !mask) final_dist = dist;
            }
            stopped = stopped || mask != 0ull;
            if (b + lanes <= T) {      // another pass: the base moves on by `lanes` ticks, a joint per lane
                demo_wave_order();
                for (int m = lane; m < A; m += 64) {
                    const float* j = model + CH_HDR + m * CH_JNT;
                    const float u = a1[m], v = a2[m];
                    float q = base[m], vel = base[A + 6 + m];
                    for (int k = b; k < b + lanes; ++k) demo_tick(j, k < n1 ? u : v, q, vel);
                    base[m] = q;
                    base[A + 6 + m] = vel;
                }
                demo_wave_order();
            }
        }
    }
    if (!wave0) return;      // (behind the last barrier; wave 0 is whole: the lanes that walked nothing hold the identities)
    for (int off = 32; off > 0; off >>= 1) {
        min_clear = fminf(min_clear, __shfl_xor(min_clear, off));
        min_self = fminf(min_self, __shfl_xor(min_self, off));
        min_cell = fminf(min_cell, __shfl_xor(min_cell, off));
        first_key = min(first_key, __shfl_xor(first_key, off));
        final_dist = fmaxf(final_dist, __shfl_xor(final_dist, off));
    }
    if (threadIdx.x != 0) return;
    float* r = records_out + n * NAF_CHAIN_DEMO_FLOATS;
    r[0] = first_key == INT_MAX ? (float)T : (float)(first_key / 8 + 1);
    r[1] = first_key == INT_MAX ? (T < n12 ? 0.f : 5.f) : (float)(first_key % 8);
    r[2] = final_dist;
    r[3] = min_clear;
    r[4] = min_self;
    r[5] = min_cell;
    r[6] = (float)n12;
    r[7] = 0.f;
}

extern "C" int naf_chain_demo_rows(naf_chain_env_t* h, const float* q_start_dev, const float* leg_actions_dev, const int32_t* n_ticks_dev,
                                   const float* targets_dev, const float* obstacles_dev, float obstacle_radius, int N, int T_cap,
                                   float* rows_out, int row_floats, float* records_out, float* poses_out, void* stream) {
    if (!h || !q_start_dev || !leg_actions_dev || !n_ticks_dev || !targets_dev || !obstacles_dev || !rows_out || !records_out)
        return NAF_ERR_ARG;
    if (N < 1 || N > 1 << 30 || T_cap < 1 || T_cap > NAF_CHAIN_DEMO_MAX_TICKS) return NAF_ERR_ARG;
    if (row_floats <= 0 || row_floats != naf_replay_row_floats(2 * h->A + 9, h->A)) return NAF_ERR_ARG;
    if (!std::isfinite(obstacle_radius) || obstacle_radius < 0.f) return NAF_ERR_ARG;
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        ChShape w = ch_shape<sc()>(h, h->waves);
        w.lds += (size_t)ch_demo_base_floats(h->A) * sizeof(float);      // the probe's rows and the base behind them
        return ch_launch_raising<chain_demo_rows_kernel<sc(), decltype(cell)...>>(
            CH_MAX_DYN_LDS + 1024, (unsigned)N, w, stream, h->model_dev, q_start_dev, leg_actions_dev, n_ticks_dev, targets_dev,
            obstacles_dev, obstacle_radius, T_cap, h->A, h->n_seg, w.n_pairs, w.lanes, row_floats, rows_out, records_out, poses_out, cell...);
    });
}

// ---- demonstrations along polylines of any number of legs (include/naf_hip.h, "Demonstrations along K legs") -----------------------
// chain_demo_rows_kernel with "leg 1 then leg 2" replaced by a schedule: ends[l] = the ticks of legs 0 .. l, staged once in LDS behind
// the base by thread 0 (at most NAF_CHAIN_DEMO_MAX_LEGS ints). Tick k belongs to the first leg whose end lies beyond it; a leg of 0
// ticks — the padding behind a query's last — has the end of the leg before it and is stepped over, and the search stops at leg
// K - 1. A tick loop keeps a leg index that only grows and reloads the leg's action only when the index changes; it starts from
// the leg of the pass's first tick, which wave 0 carries from pass to pass beside the leg of the tick before it (row b - 1's
// action is that leg's). Both are uniform. The ends are only read by wave 0, behind the demo_wave_order that orders the base.
__device__ static inline int demo_leg_of(const int* ends, int K, int l, int k) {      // the leg of tick k, searched upwards from leg l
    while (l < K - 1 && k >= ends[l]) ++l;
    return l;
}

// ticks k0 .. k1 - 1 of joint m from the leg l of tick k0; acts = leg_actions[n] + m, a leg A floats on
__device__ static inline void demo_run_legs(const float* j, const float* acts, int A, const int* ends, int K, int l, int k0, int k1,
                                            float& q, float& vel) {
    int end = ends[l];
    float u = acts[l * A];
    for (int k = k0; k < k1; ++k) {
        if (k >= end && l < K - 1) {
            do end = ends[++l];
            while (k >= end && l < K - 1);
            u = acts[l * A];
        }
        demo_tick(j, u, q, vel);
    }
}

template <bool SC, class... Cell>
__global__ void __launch_bounds__(SC ? 64 * CH_MAX_WAVES : 64)
chain_demo_legs_kernel(const float* __restrict__ model, const float* __restrict__ q_start, const float* __restrict__ leg_actions,
                       const int* __restrict__ n_ticks, int K, const float* __restrict__ targets, const float* __restrict__ obstacles,
                       float orad, int T_cap, int A, int n_seg, int n_pairs, int lanes, int row_floats, float* __restrict__ rows_out,
                       float* __restrict__ records_out, float* __restrict__ poses_out, const Cell... cell) {
    constexpr bool CELL = (std::is_same_v<Cell, ChainCell> || ... || false);
    constexpr bool BOX = (std::is_same_v<Cell, ChainBox> || ... || false);
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    const int64_t n = blockIdx.x;
    const int S = 2 * A + 9;
    const int off_s2 = naf_row_off_s2(S, A), off_d = naf_row_off_done(S, A);
    const float* acts = leg_actions + n * K * A;
    const float ox = obstacles[n * 3], oy = obstacles[n * 3 + 1], oz = obstacles[n * 3 + 2];
    const float tx = targets[n * 3], ty = targets[n * 3 + 1], tz = targets[n * 3 + 2];
    const int lane = threadIdx.x & 63;
    const bool active = lane < lanes;
    const bool wave0 = threadIdx.x < 64;
    float* base = ch_lds + (SC ? ch_lds_bytes(n_seg, lanes, blockDim.x >> 6) / sizeof(float) : 0);
    int* ends = (int*)(base + ch_demo_base_floats(A));
    // (the host validated the counts; the clamps only keep a wrong upload inside the arrays. Every thread sums them: T is uniform)
    int total = 0;
    for (int l = 0; l < K; ++l) {
        total += min(max(n_ticks[n * K + l], l == 0 ? 1 : 0), 1 << 20);
        if (threadIdx.x == 0) ends[l] = total;
    }
    const int T = min(total, T_cap);                     // rows of this demonstration; poses 0 .. T
    float* rows = rows_out + n * T_cap * row_floats;
    if (wave0) {
        for (int m = lane; m < A; m += 64) {
            const float* j = model + CH_HDR + m * CH_JNT;
            float q = q_start[n * A + m];
            if (j[16] != 0.f) {      // p_0: the start pose clamped into the limits, as naf_chain_env_reset_given clamps it
                if (q > j[18]) q = j[18];
                if (q < j[17]) q = j[17];
            }
            base[m] = q;
            base[A + 6 + m] = 0.f;
        }
        if (lane < 3) {
            base[A + lane] = targets[n * 3 + lane];
            base[A + 3 + lane] = obstacles[n * 3 + lane];
        }
        demo_wave_order();
    }
    float min_clear = INFINITY, min_self = INFINITY, min_cell = INFINITY, final_dist = -1.f;
    int first_key = INT_MAX;      // 8 x (row of the first done) + its end code
    bool stopped = false;         // (uniform in wave 0) a pass before this one held the first done
    int leg_b = 0, leg_prev = 0;  // (uniform in wave 0) the legs of tick b and of tick max(b - 1, 0)
    for (int b = 0; b <= T; b += lanes) {      // (uniform: every thread takes every pass)
        const int t = b + lane;
        const bool walks = active && wave0 && t <= T;
        float* prev = rows + (int64_t)(t - 1) * row_floats;      // row t - 1: used only where t >= 1
        float* o = t < T ? prev + row_floats : prev + off_s2;    // obs(p_t): row t's state, or the last row's next_state
        float ee[3];
        bool hit = false;
        WalkAux aux = {SC ? ch_lds + lane : nullptr, lanes, INFINITY, INFINITY};
        if (walks) {
            float* rec = poses_out ? poses_out + ((n * (T_cap + 1)) + t) * A : nullptr;
            hit = chain_walk_at<SC, false, false, true, CELL, BOX>(
                model, A, n_seg,
                [=](int m) {
                    const float* j = model + CH_HDR + m * CH_JNT;
                    float q = base[m], vel = base[A + 6 + m];
                    demo_run_legs(j, acts + m, A, ends, K, leg_b, b, t, q, vel);
                    const int slot = (int)j[21];
                    if (slot >= 0) o[A + slot] = vel;      // what step t - 1 reported (0 at t = 0, 0 where a limit stopped the joint)
                    if (rec) rec[m] = q;
                    return q;
                },
                ox, oy, oz, orad, base, o, ee, aux);
        }
        float self_clear = INFINITY;
        if constexpr (SC) self_clear = self_clearance_phase(model, A, n_seg, n_pairs, ch_lds, lanes, lane, active && t <= T);
        if (wave0) {
            const bool outcome = walks && t >= 1;      // the walk of p_t is the outcome of row t - 1
            float dist = 0.f, clear = INFINITY, cellc = INFINITY;
            bool done = false;
            int code = 0;
            if (outcome) {
                const float dx = ee[0] - tx, dy = ee[1] - ty, dz = ee[2] - tz;
                dist = sqrtf(dx * dx + dy * dy + dz * dz);
                clear = aux.clear - orad;
                if constexpr (CELL) cellc = aux.cell;
                const bool reached = dist < CH_REACHED, self_hit = self_clear < 0.f, cell_hit = CELL && aux.cell < 0.f;
                const bool any = hit || self_hit || cell_hit;
                done = reached || any;
                code = reached ? 1 : (hit ? 2 : (self_hit ? 3 : (cell_hit ? 4 : 0)));
                const float* act = acts + demo_leg_of(ends, K, leg_prev, t - 1) * A;      // the action of tick t - 1's leg
                for (int m = 0; m < A; ++m) prev[S + m] = act[m];
                prev[S + A] = reached ? 250.f : (any ? -1000.f : -(dist - CH_REACHED));
                for (int k = S + A + 1; k < off_s2; ++k) prev[k] = 0.f;
                if (t < T)
                    for (int k = 0; k < S; ++k) prev[off_s2 + k] = o[k];
                prev[off_d] = done ? 1.f : 0.f;
                for (int k = off_d + 1; k < row_floats; ++k) prev[k] = 0.f;      // the tag float included: an untagged row
            }
            const unsigned long long mask = __ballot(outcome && done);
            const int first_lane = mask ? __ffsll(mask) - 1 : 64;
            if (!stopped && outcome && lane <= first_lane) {      // rows up to the first done are the demonstration's
                min_clear = fminf(min_clear, clear);
                min_self = fminf(min_self, self_clear);
                min_cell = fminf(min_cell, cellc);
                if (lane == first_lane) { first_key = (t - 1) * 8 + code; final_dist = dist; }
                else if (t == T && !mask) final_dist = dist;
            }
            stopped = stopped || mask != 0ull;
            if (b + lanes <= T) {      // another pass: the base moves on by `lanes` ticks, a joint per lane
                demo_wave_order();
                for (int m = lane; m < A; m += 64) {
                    const float* j = model + CH_HDR + m * CH_JNT;
                    float q = base[m], vel = base[A + 6 + m];
                    demo_run_legs(j, acts + m, A, ends, K, leg_b, b, b + lanes, q, vel);
                    base[m] = q;
                    base[A + 6 + m] = vel;
                }
                leg_prev = demo_leg_of(ends, K, leg_b, b + lanes - 1);
                leg_b = demo_leg_of(ends, K, leg_prev, b + lanes);
                demo_wave_order();
            }
        }
    }
    if (!wave0) return;      // (behind the last barrier; wave 0 is whole: the lanes that walked nothing hold the identities)
    for (int off = 32; off > 0; off >>= 1) {
        min_clear = fminf(min_clear, __shfl_xor(min_clear, off));
        min_self = fminf(min_self, __shfl_xor(min_self, off));
        min_cell = fminf(min_cell, __shfl_xor(min_cell, off));
        first_key = min(first_key, __shfl_xor(first_key, off));
        final_dist = fmaxf(final_dist, __shfl_xor(final_dist, off));
    }
    if (threadIdx.x != 0) return;
    float* r = records_out + n * NAF_CHAIN_DEMO_FLOATS;
    r[0] = first_key == INT_MAX ? (float)T : (float)(first_key / 8 + 1);
    r[1] = first_key == INT_MAX ? (T < total ? 0.f : 5.f) : (float)(first_key % 8);
    r[2] = final_dist;
    r[3] = min_clear;
    r[4] = min_self;
    r[5] = min_cell;
    r[6] = (float)total;
    r[7] = 0.f;
}

extern "C" int naf_chain_demo_rows_legs(naf_chain_env_t* h, const float* q_start_dev, const float* leg_actions_dev,
                                        const int32_t* n_ticks_dev, int K, const float* targets_dev, const float* obstacles_dev,
                                        float obstacle_radius, int N, int T_cap, float* rows_out, int row_floats, float* records_out,
                                        float* poses_out, void* stream) {
    if (!h || !q_start_dev || !leg_actions_dev || !n_ticks_dev || !targets_dev || !obstacles_dev || !rows_out || !records_out)
        return NAF_ERR_ARG;
    if (K < 1 || K > NAF_CHAIN_DEMO_MAX_LEGS) return NAF_ERR_ARG;
    if (N < 1 || N > 1 << 30 || T_cap < 1 || T_cap > NAF_CHAIN_DEMO_MAX_TICKS) return NAF_ERR_ARG;
    if (row_floats <= 0 || row_floats != naf_replay_row_floats(2 * h->A + 9, h->A)) return NAF_ERR_ARG;
    if (!std::isfinite(obstacle_radius) || obstacle_radius < 0.f) return NAF_ERR_ARG;
    return ch_with_pack(h, [&](auto sc, auto... cell) {
        ChShape w = ch_shape<sc()>(h, h->waves);
        // the probe's rows, the base behind them and the K ends behind the base
        w.lds += (size_t)ch_demo_base_floats(h->A) * sizeof(float) + (size_t)K * sizeof(int);
        return ch_launch_raising<chain_demo_legs_kernel<sc(), decltype(cell)...>>(
            CH_MAX_DYN_LDS + 1024 + NAF_CHAIN_DEMO_MAX_LEGS * (int)sizeof(int), (unsigned)N, w, stream, h->model_dev, q_start_dev,
            leg_actions_dev, n_ticks_dev, K, targets_dev, obstacles_dev, obstacle_radius, T_cap, h->A, h->n_seg, w.n_pairs, w.lanes,
            row_floats, rows_out, records_out, poses_out, cell...);
    });
}

// ---- demonstrations under one action per tick (include/naf_hip.h, "Demonstrations under per-tick actions") ------------------------
// chain_demo_legs_kernel with the schedule replaced by a table: tick k of demonstration n applies tick_actions[n][k], an action of
// its own. A THIRD kernel beside the two, not a template argument of one body: the two existing symbols keep their instructions
// (DESIGN §28). The base-pose recurrence is theirs. The action of tick k comes from a per-pass table in LDS behind the base —
// table[lanes][A], the actions of ticks b .. b + lanes - 1 — staged by wave 0 before the pass with coalesced loads, bounded by
// T_n x A so that nothing behind a demonstration's own ticks is read; in the accessor's tick loop every lane reads the same (k, m)
// word, an LDS broadcast. Row t - 1's action is table row lane - 1; for lane 0 of a pass it is the last row of the PREVIOUS pass's
// table, kept as row -1 (A floats in front of the table) before the table is staged again. Only wave 0 touches the table, in
// program order, behind demo_wave_order as the base is.
template <bool SC, class... Cell>
__global__ void __launch_bounds__(SC ? 64 * CH_MAX_WAVES : 64)
chain_demo_ticks_kernel(const float* __restrict__ model, const float* __restrict__ q_start, const float* __restrict__ tick_actions,
                        const int* __restrict__ n_ticks, const float* __restrict__ targets, const float* __restrict__ obstacles,
                        float orad, int T_cap, int A, int n_seg, int n_pairs, int lanes, int row_floats, float* __restrict__ rows_out,
                        float* __restrict__ records_out, float* __restrict__ poses_out, const Cell... cell) {
    constexpr bool CELL = (std::is_same_v<Cell, ChainCell> || ... || false);
    constexpr bool BOX = (std::is_same_v<Cell, ChainBox> || ... || false);
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    const int64_t n = blockIdx.x;
    const int S = 2 * A + 9;
    const int off_s2 = naf_row_off_s2(S, A), off_d = naf_row_off_done(S, A);
    // (the host validated the count; the clamp only keeps a wrong upload inside the arrays)
    const int planned = min(max(n_ticks[n], 1), 1 << 20);
    const int T = min(planned, T_cap);                   // rows of this demonstration; poses 0 .. T
    const float ox = obstacles[n * 3], oy = obstacles[n * 3 + 1], oz = obstacles[n * 3 + 2];
    const float tx = targets[n * 3], ty = targets[n * 3 + 1], tz = targets[n * 3 + 2];
    const int lane = threadIdx.x & 63;
    const bool active = lane < lanes;
    const bool wave0 = threadIdx.x < 64;
    float* base = ch_lds + (SC ? ch_lds_bytes(n_seg, lanes, blockDim.x >> 6) / sizeof(float) : 0);
    float* table = base + ch_demo_base_floats(A) + A;      // row -1, the A floats in front of it, is the carry
    float* rows = rows_out + n * T_cap * row_floats;
    if (wave0) {
        for (int m = lane; m < A; m += 64) {
            const float* j = model + CH_HDR + m * CH_JNT;
            float q = q_start[n * A + m];
            if (j[16] != 0.f) {      // p_0: the start pose clamped into the limits, as naf_chain_env_reset_given clamps it
                if (q > j[18]) q = j[18];
                if (q < j[17]) q = j[17];
            }
            base[m] = q;
            base[A + 6 + m] = 0.f;
        }
        if (lane < 3) {
            base[A + lane] = targets[n * 3 + lane];
            base[A + 3 + lane] = obstacles[n * 3 + lane];
        }
        demo_wave_order();
    }
    float min_clear = INFINITY, min_self = INFINITY, min_cell = INFINITY, final_dist = -1.f;
    int first_key = INT_MAX;      // 8 x (row of the first done) + its end code
    bool stopped = false;         // (uniform in wave 0) a pass before this one held the first done
    for (int b = 0; b <= T; b += lanes) {      // (uniform: every thread takes every pass)
        const int t = b + lane;
        if (wave0) {      // the pass's actions: the last one of the pass before into the carry, then ticks b .. b + lanes - 1 below T
            if (b > 0) {
                for (int m = lane; m < A; m += 64) table[m - A] = table[(lanes - 1) * A + m];
                demo_wave_order();
            }
            const float* pass = tick_actions + (n * T_cap + b) * A;
            for (int i = lane; i < min(lanes, T - b) * A; i += 64) table[i] = pass[i];
            demo_wave_order();
        }
        const bool walks = active && wave0 && t <= T;
        float* prev = rows + (int64_t)(t - 1) * row_floats;      // row t - 1: used only where t >= 1
        float* o = t < T ? prev + row_floats : prev + off_s2;    // obs(p_t): row t's state, or the last row's next_state
        float ee[3];
        bool hit = false;
        WalkAux aux = {SC ? ch_lds + lane : nullptr, lanes, INFINITY, INFINITY};
        if (walks) {
            hit = chain_walk_at<SC, false, false, true, CELL, BOX>(
                model, A, n_seg,
                [=](int m) {
                    const float* j = model + CH_HDR + m * CH_JNT;
                    float q = base[m], vel = base[A + 6 + m];
                    for (int k = 0; k < lane; ++k) demo_tick(j, table[k * A + m], q, vel);      // ticks b .. t - 1
                    const int slot = (int)j[21];
                    if (slot >= 0) o[A + slot] = vel;      // what step t - 1 reported (0 at t = 0, 0 where a limit stopped the joint)
                    if (poses_out) poses_out[((n * (T_cap + 1)) + t) * A + m] = q;
                    return q;
                },
                ox, oy, oz, orad, base, o, ee, aux);
        }
        float self_clear = INFINITY;
        if constexpr (SC) self_clear = self_clearance_phase(model, A, n_seg, n_pairs, ch_lds, lanes, lane, active && t <= T);
        if (wave0) {
            const bool outcome = walks && t >= 1;      // the walk of p_t is the outcome of row t - 1
            float dist = 0.f, clear = INFINITY, cellc = INFINITY;
            bool done = false;
            int code = 0;
            if (outcome) {
                const float dx = ee[0] - tx, dy = ee[1] - ty, dz = ee[2] - tz;
                dist = sqrtf(dx * dx + dy * dy + dz * dz);
                clear = aux.clear - orad;
                if constexpr (CELL) cellc = aux.cell;
                const bool reached = dist < CH_REACHED, self_hit = self_clear < 0.f, cell_hit = CELL && aux.cell < 0.f;
                const bool any = hit || self_hit || cell_hit;
                done = reached || any;
                code = reached ? 1 : (hit ? 2 : (self_hit ? 3 : (cell_hit ? 4 : 0)));
                const float* act = table + (lane - 1) * A;      // the action of tick t - 1: for lane 0 the carry
                for (int m = 0; m < A; ++m) prev[S + m] = act[m];
                prev[S + A] = reached ? 250.f : (any ? -1000.f : -(dist - CH_REACHED));
                for (int k = S + A + 1; k < off_s2; ++k) prev[k] = 0.f;
                if (t < T)
                    for (int k = 0; k < S; ++k) prev[off_s2 + k] = o[k];
                prev[off_d] = done ? 1.f : 0.f;
                for (int k = off_d + 1; k < row_floats; ++k) prev[k] = 0.f;      // the tag float included: an untagged row
            }
            const unsigned long long mask = __ballot(outcome && done);
            const int first_lane = mask ? __ffsll(mask) - 1 : 64;
            if (!stopped && outcome && lane <= first_lane) {      // rows up to the first done are the demonstration's
                min_clear = fminf(min_clear, clear);
                min_self = fminf(min_self, self_clear);
                min_cell = fminf(min_cell, cellc);
                if (lane == first_lane) { first_key = (t - 1) * 8 + code; final_dist = dist; }
                else if (t == T && !mask) final_dist = dist;
            }
            stopped = stopped || mask != 0ull;
            if (b + lanes <= T) {      // another pass: the base moves on by `lanes` ticks, a joint per lane
                demo_wave_order();
                for (int m = lane; m < A; m += 64) {
                    const float* j = model + CH_HDR + m * CH_JNT;
                    float q = base[m], vel = base[A + 6 + m];
                    for (int k = 0; k < lanes; ++k) demo_tick(j, table[k * A + m], q, vel);      // ticks b .. b + lanes - 1, all below T
                    base[m] = q;
                    base[A + 6 + m] = vel;
                }
                demo_wave_order();
            }
        }
    }
    if (!wave0) return;      // (behind the last barrier; wave 0 is whole: the lanes that walked nothing hold the identities)
    for (int off = 32; off > 0; off >>= 1) {
        min_clear = fminf(min_clear, __shfl_xor(min_clear, off));
        min_self = fminf(min_self, __shfl_xor(min_self, off));
        min_cell = fminf(min_cell, __shfl_xor(min_cell, off));
        first_key = min(first_key, __shfl_xor(first_key, off));
        final_dist = fmaxf(final_dist, __shfl_xor(final_dist, off));
    }
    if (threadIdx.x != 0) return;
    float* r = records_out + n * NAF_CHAIN_DEMO_FLOATS;
    r[0] = first_key == INT_MAX ? (float)T : (float)(first_key / 8 + 1);
    r[1] = first_key == INT_MAX ? (T < min(max(n_ticks[n], 1), 1 << 20) ? 0.f : 5.f) : (float)(first_key % 8);
    r[2] = final_dist;
    r[3] = min_clear;
    r[4] = min_self;
    r[5] = min_cell;
    r[6] = (float)min(max(n_ticks[n], 1), 1 << 20);
    r[7] = 0.f;
}

extern "C" int naf_chain_demo_rows_ticks(naf_chain_env_t* h, const float* q_start_dev, const float* tick_actions_dev,
                                         const int32_t* n_ticks_dev, const float* targets_dev, const float* obstacles_dev,
                                         float obstacle_radius, int N, int T_cap, float* rows_out, int row_floats, float* records_out,
                                         float* poses_out, void* stream) {
    if (!h || !q_start_dev || !tick_actions_dev || !n_ticks_dev || !targets_dev || !obstacles_dev || !rows_out || !records_out)
        return NAF_ERR_ARG;
    if (N < 1 || N > 1 << 30 || T_cap < 1 || T_cap > NAF_CHAIN_DEMO_MAX_TICKS) return NAF_ERR_ARG;
    if (row_floats <= 0 || row_floats != naf_replay_row_floats(2 * h->A + 9, h->A)) return NAF_ERR_ARG;
    if (!std::isfinite(obstacle_radius) || obstacle_radius < 0.f) return NAF_ERR_ARG;
    return ch_with_pack(h, [&](auto sc, auto... cell) -> int {
        ChShape w = ch_shape<sc()>(h, h->waves);
        // the probe's rows, the base behind them, one action (the carry) and the pass's lanes x A actions behind the base
        w.lds += ((size_t)ch_demo_base_floats(h->A) + (size_t)(w.lanes + 1) * h->A) * sizeof(float);
        if (w.lds > CH_WG_LDS) return NAF_CHAIN_ERR_LDS;      // (rows that only just fit 144 KiB and a wide arm's table)
        return ch_launch_raising<chain_demo_ticks_kernel<sc(), decltype(cell)...>>(
            CH_WG_LDS, (unsigned)N, w, stream, h->model_dev, q_start_dev, tick_actions_dev, n_ticks_dev, targets_dev, obstacles_dev,
            obstacle_radius, T_cap, h->A, h->n_seg, w.n_pairs, w.lanes, row_floats, rows_out, records_out, poses_out, cell...);
    });
}

// ---- goal poses pushed out of contact in the task's null space (include/naf_hip.h, "Goal poses out of contact") -------------------
// chain_ik_solve_kernel's shape — one lane per candidate, one wave per workgroup, no barrier — with a walk of ALL A joints: the
// [m][6][lane] record of (a_m, p_m) for every driven joint, and behind it the capsules' world end points as [segment][6][lane].
// Beside the end effector the walk collects the LEAST of all the clearance tests the selection compares with the margin — per
// capsule the obstacle, then the workcell geometries its mask names; after the walk the self pairs, a serial loop per lane over
// LDS — and that test's witness: a handful of registers replaced by select when a smaller test appears. The distance bodies are
// restated here with their witnesses; frame_geometry, chain_walk_at, seg_*_dist2 and the solve kernels are not touched. The counts
// P, G, H, B are the blob's header floats, uniform: a loop runs zero times where its section is absent, and the mask and geometry
// sections are not addressed in a blob without a workcell. environment/kinematic.py (least_test, clearance_gradient, ik_clear_step,
// refine_goal_poses) is the float64 statement.
#define IKC_SIGMA_FLOOR 1e-6f
#define IKC_WITNESS_FLOOR 1e-6f      // (a micrometre: float32 leaves some 1e-8 of a zero distance between points half a metre out)

struct ClearWitness {
    float c;                     // the running least clearance
    int kind, f, f2;             // 0 obstacle / 1 self / 2 workcell; the capsule's frame; a pair's second frame (0: no joint moves it)
    float x0, x1, x2;            // the point on the capsule's axis where the distance is attained
    float n0, n1, n2;            // the unit direction from the geometry's nearest point to x (0: no gradient)
    float y0, y1, y2;            // a pair's second point
};

__device__ __forceinline__ void ikc_offer(ClearWitness& w, float c, int kind, int f, float x0, float x1, float x2, float d0, float d1,
                                          float d2, float dist, int f2 = 0, float y0 = 0.f, float y1 = 0.f, float y2 = 0.f) {
    const bool take = c < w.c;
    const float inv = dist >= IKC_WITNESS_FLOOR ? 1.f / dist : 0.f;
    w.c = take ? c : w.c;
    w.kind = take ? kind : w.kind;
    w.f = take ? f : w.f;
    w.f2 = take ? f2 : w.f2;
    w.x0 = take ? x0 : w.x0; w.x1 = take ? x1 : w.x1; w.x2 = take ? x2 : w.x2;
    w.n0 = take ? d0 * inv : w.n0; w.n1 = take ? d1 * inv : w.n1; w.n2 = take ? d2 * inv : w.n2;
    w.y0 = take ? y0 : w.y0; w.y1 = take ? y1 : w.y1; w.y2 = take ? y2 : w.y2;
}

// seg_point_dist2 with its witness: the clamped projection parameter
__device__ __forceinline__ float ikc_seg_point(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                               float& t_out) {
    const float ux = bx - ax, uy = by - ay, uz = bz - az;
    const float wx = cx - ax, wy = cy - ay, wz = cz - az;
    const float den = ux * ux + uy * uy + uz * uz;
    float t = den > 0.f ? (wx * ux + wy * uy + wz * uz) / den : 0.f;
    t = fminf(1.f, fmaxf(0.f, t));
    const float dx = wx - t * ux, dy = wy - t * uy, dz = wz - t * uz;
    t_out = t;
    return dx * dx + dy * dy + dz * dz;
}

// a capsule's axis a-b against the sphere (centre c, radius rad): the test d - rad - rho and its witness
__device__ __forceinline__ void ikc_sphere(ClearWitness& w, int kind, int f, float ax, float ay, float az, float bx, float by, float bz,
                                           float cx, float cy, float cz, float rad, float rho) {
    float t;
    const float d = sqrtf(ikc_seg_point(ax, ay, az, bx, by, bz, cx, cy, cz, t));
    const float x0 = ax + t * (bx - ax), x1 = ay + t * (by - ay), x2 = az + t * (bz - az);
    ikc_offer(w, d - rad - rho, kind, f, x0, x1, x2, x0 - cx, x1 - cy, x2 - cz, d);
}

// seg_box_dist2 with its witness: the parameter t it ends with
__device__ static inline float ikc_seg_box(float px, float py, float pz, float ux, float uy, float uz, float hx, float hy, float hz,
                                           float& t_out) {
    float t_lo = 0.f, t_hi = 1.f;
    float g_lo = box_slope(0.f, px, py, pz, ux, uy, uz, hx, hy, hz), g_hi = box_slope(1.f, px, py, pz, ux, uy, uz, hx, hy, hz);
    const float g0 = g_lo, g1 = g_hi;
    const float p[3] = {px, py, pz}, u[3] = {ux, uy, uz}, h[3] = {hx, hy, hz};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int i = k >> 1;
        const float inv = u[i] != 0.f ? 1.f / u[i] : 0.f;
        const float t = fminf(1.f, fmaxf(0.f, ((k & 1 ? h[i] : -h[i]) - p[i]) * inv));
        const float g = box_slope(t, px, py, pz, ux, uy, uz, hx, hy, hz);
        const bool lo = g <= 0.f && t >= t_lo, hi = g >= 0.f && t <= t_hi;
        t_lo = lo ? t : t_lo;
        g_lo = lo ? g : g_lo;
        t_hi = hi ? t : t_hi;
        g_hi = hi ? g : g_hi;
    }
    const float den = g_hi - g_lo;
    float t = den > 0.f ? t_lo - g_lo * (t_hi - t_lo) / den : t_lo;
    t = fminf(t_hi, fmaxf(t_lo, t));
    t = g0 > 0.f ? 0.f : (g1 < 0.f ? 1.f : t);
    t_out = t;
    const float x = fmaf(t, ux, px), y = fmaf(t, uy, py), z = fmaf(t, uz, pz);
    const float ex = fmaxf(fabsf(x) - hx, 0.f), ey = fmaxf(fabsf(y) - hy, 0.f), ez = fmaxf(fabsf(z) - hz, 0.f);
    return ex * ex + ey * ey + ez * ez;
}

// the tests of frame f's capsules — the obstacle, then the masked workcell geometries — and their end points into LDS
__device__ static inline void ikc_frame(const float* __restrict__ model, int A, int n_seg, int f, const Frame& F, float ox, float oy,
                                        float oz, float orad, float* ends, ClearWitness& w) {
    const float* begin = model + ch_off_begin(A);
    const float* segs = model + ch_off_seg(A);
    const int s0 = (int)begin[f], s1 = (int)begin[f + 1];
    const int n_sph = (int)model[10], n_geo = n_sph + (int)model[11], n_box = (int)model[12];
    const float* geo = model + ch_off_cell(A, n_seg, (int)model[9]);      // (addressed only when n_geo + n_box > 0)
    for (int s = s0; s < s1; ++s) {
        const float* g = segs + s * CH_SEG;
        const float ax = F.px + F.r00 * g[1] + F.r01 * g[2] + F.r02 * g[3];
        const float ay = F.py + F.r10 * g[1] + F.r11 * g[2] + F.r12 * g[3];
        const float az = F.pz + F.r20 * g[1] + F.r21 * g[2] + F.r22 * g[3];
        const float bx = F.px + F.r00 * g[4] + F.r01 * g[5] + F.r02 * g[6];
        const float by = F.py + F.r10 * g[4] + F.r11 * g[5] + F.r12 * g[6];
        const float bz = F.pz + F.r20 * g[4] + F.r21 * g[5] + F.r22 * g[6];
        float* e = ends + (size_t)s * 6 * 64;
        e[0] = ax; e[64] = ay; e[128] = az;
        e[192] = bx; e[256] = by; e[320] = bz;
        ikc_sphere(w, 0, f, ax, ay, az, bx, by, bz, ox, oy, oz, orad, g[7]);
        if (n_geo + n_box == 0) continue;
        const int mask = (int)geo[4 * n_geo + CH_BOX * n_box + s];
        for (int k = 0; k < n_geo; ++k) {      // (uniform: the counts, the mask and the geometry are the blob's)
            if (!(mask >> k & 1)) continue;
            const float* c = geo + 4 * k;
            if (k < n_sph) {
                ikc_sphere(w, 2, f, ax, ay, az, bx, by, bz, c[0], c[1], c[2], c[3], g[7]);
            } else {      // the end point with the smaller n . x; the direction is the plane's normal
                const float na = c[0] * ax + c[1] * ay + c[2] * az, nb = c[0] * bx + c[1] * by + c[2] * bz;
                const bool first = na <= nb;
                ikc_offer(w, fminf(na, nb) - c[3] - g[7], 2, f, first ? ax : bx, first ? ay : by, first ? az : bz, c[0], c[1], c[2], 1.f);
            }
        }
        const int bmask = mask >> n_geo;
        const float wx = bx - ax, wy = by - ay, wz = bz - az;
        for (int k = 0; k < n_box; ++k) {      // (uniform, as above)
            if (!(bmask >> k & 1)) continue;
            const float* x = geo + 4 * n_geo + CH_BOX * k;      // c | R row-major | h | r
            const float ex = ax - x[0], ey = ay - x[1], ez = az - x[2];
            const float px = x[3] * ex + x[6] * ey + x[9] * ez, py = x[4] * ex + x[7] * ey + x[10] * ez,
                        pz = x[5] * ex + x[8] * ey + x[11] * ez;
            const float ux = x[3] * wx + x[6] * wy + x[9] * wz, uy = x[4] * wx + x[7] * wy + x[10] * wz,
                        uz = x[5] * wx + x[8] * wy + x[11] * wz;
            float t;
            const float d = sqrtf(ikc_seg_box(px, py, pz, ux, uy, uz, x[12], x[13], x[14], t));
            // the point at t in the box's frame minus its clamp into the box, rotated back to the world
            const float lx = fmaf(t, ux, px), ly = fmaf(t, uy, py), lz = fmaf(t, uz, pz);
            const float dx = lx - fminf(x[12], fmaxf(-x[12], lx)), dy = ly - fminf(x[13], fmaxf(-x[13], ly)),
                        dz = lz - fminf(x[14], fmaxf(-x[14], lz));
            ikc_offer(w, d - x[15] - g[7], 2, f, ax + t * wx, ay + t * wy, az + t * wz, x[3] * dx + x[4] * dy + x[5] * dz,
                      x[6] * dx + x[7] * dy + x[8] * dz, x[9] * dx + x[10] * dy + x[11] * dz, d);
        }
    }
}

// walks all A joints at q: (a_m, p_m) of every joint to ax[(m * 6 + k) * 64], the capsules' end points to `ends`, the end effector
// to ee, the least obstacle / workcell test and its witness to w
__device__ static inline void ikc_walk(const float* __restrict__ model, int A, int n_seg, const float* q, float ox, float oy, float oz,
                                       float orad, float* ax, float* ends, float* ee, ClearWitness& w) {
    const int ee_frame = (int)model[4];
    Frame F = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    w.c = INFINITY;
    w.kind = w.f = w.f2 = 0;
    w.x0 = w.x1 = w.x2 = w.n0 = w.n1 = w.n2 = w.y0 = w.y1 = w.y2 = 0.f;
    ee[0] = ee[1] = ee[2] = 0.f;
    for (int f = 0;; ++f) {
        ikc_frame(model, A, n_seg, f, F, ox, oy, oz, orad, ends, w);
        if (f == ee_frame) {
            ee[0] = F.px + F.r00 * model[5] + F.r01 * model[6] + F.r02 * model[7];
            ee[1] = F.py + F.r10 * model[5] + F.r11 * model[6] + F.r12 * model[7];
            ee[2] = F.pz + F.r20 * model[5] + F.r21 * model[6] + F.r22 * model[7];
        }
        if (f == A) break;
        const int m = f;
        const float* j = model + CH_HDR + m * CH_JNT;
        const float qm = q[m];
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
        const float wx = G.r00 * x + G.r01 * y + G.r02 * z, wy = G.r10 * x + G.r11 * y + G.r12 * z,
                    wz = G.r20 * x + G.r21 * y + G.r22 * z;
        float* rec = ax + m * 6 * 64;
        rec[0] = wx; rec[64] = wy; rec[128] = wz;
        rec[192] = F.px; rec[256] = F.py; rec[320] = F.pz;
        if (j[15] != 0.f) {      // prismatic
            F.r00 = G.r00; F.r01 = G.r01; F.r02 = G.r02;
            F.r10 = G.r10; F.r11 = G.r11; F.r12 = G.r12;
            F.r20 = G.r20; F.r21 = G.r21; F.r22 = G.r22;
            F.px += wx * qm;
            F.py += wy * qm;
            F.pz += wz * qm;
        } else {                 // revolute: chain_walk's Rodrigues form
            float s, c;
            sincosf(qm, &s, &c);
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
    }
}

// the self pairs, a serial loop over the lane's end points in LDS: seg_seg_dist2's five candidates with their parameters, the
// least of them (ties to the first) the pair's witness
__device__ static inline void ikc_pairs(const float* __restrict__ model, int A, int n_seg, int n_pairs, const float* ends,
                                        ClearWitness& w) {
    const float* segs = model + ch_off_seg(A);
    const float* pairs = model + ch_off_pair(A, n_seg);      // (addressed only when n_pairs > 0)
    for (int p = 0; p < n_pairs; ++p) {
        const int s = (int)pairs[2 * p], t_ = (int)pairs[2 * p + 1];
        const float* e = ends + (size_t)s * 6 * 64;
        const float* g = ends + (size_t)t_ * 6 * 64;
        const float ax = e[0], ay = e[64], az = e[128], bx = e[192], by = e[256], bz = e[320];
        const float cx = g[0], cy = g[64], cz = g[128], dx = g[192], dy = g[256], dz = g[320];
        const float ux = bx - ax, uy = by - ay, uz = bz - az;
        const float vx = dx - cx, vy = dy - cy, vz = dz - cz;
        const float wx = ax - cx, wy = ay - cy, wz = az - cz;
        const float a = ux * ux + uy * uy + uz * uz, b = ux * vx + uy * vy + uz * vz, c = vx * vx + vy * vy + vz * vz;
        const float d = ux * wx + uy * wy + uz * wz, ee_ = vx * wx + vy * wy + vz * wz;
        const float den = a * c - b * b;
        float sp = den > 1e-7f * a * c ? (b * ee_ - c * d) / den : 0.f;
        sp = fminf(1.f, fmaxf(0.f, sp));
        float tp = c > 0.f ? (b * sp + ee_) / c : 0.f;
        tp = fminf(1.f, fmaxf(0.f, tp));
        sp = a > 0.f ? (b * tp - d) / a : 0.f;
        sp = fminf(1.f, fmaxf(0.f, sp));
        const float xx = wx + sp * ux - tp * vx, xy = wy + sp * uy - tp * vy, xz = wz + sp * uz - tp * vz;
        float best = xx * xx + xy * xy + xz * xz, t;
        float d2 = ikc_seg_point(cx, cy, cz, dx, dy, dz, ax, ay, az, t);
        bool take = d2 < best;
        sp = take ? 0.f : sp; tp = take ? t : tp; best = take ? d2 : best;
        d2 = ikc_seg_point(cx, cy, cz, dx, dy, dz, bx, by, bz, t);
        take = d2 < best;
        sp = take ? 1.f : sp; tp = take ? t : tp; best = take ? d2 : best;
        d2 = ikc_seg_point(ax, ay, az, bx, by, bz, cx, cy, cz, t);
        take = d2 < best;
        sp = take ? t : sp; tp = take ? 0.f : tp; best = take ? d2 : best;
        d2 = ikc_seg_point(ax, ay, az, bx, by, bz, dx, dy, dz, t);
        take = d2 < best;
        sp = take ? t : sp; tp = take ? 1.f : tp; best = take ? d2 : best;
        const float x0 = ax + sp * ux, x1 = ay + sp * uy, x2 = az + sp * uz;
        const float y0 = cx + tp * vx, y1 = cy + tp * vy, y2 = cz + tp * vz;
        const float e0 = x0 - y0, e1 = x1 - y1, e2 = x2 - y2;
        const float dist = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
        ikc_offer(w, dist - (segs[s * CH_SEG + 7] + segs[t_ * CH_SEG + 7]), 1, (int)segs[s * CH_SEG], x0, x1, x2, e0, e1, e2, dist,
                  (int)segs[t_ * CH_SEG], y0, y1, y2);
    }
}

// joint m's task column c and its entry gamma of the least test's gradient, from its LDS record
__device__ __forceinline__ float ikc_column(const float* __restrict__ model, int m, int n_joints, const float* ax, const float* ee,
                                            const ClearWitness& w, float* c) {
    const float* r = ax + m * 6 * 64;
    const float a0 = r[0], a1 = r[64], a2 = r[128], p0 = r[192], p1 = r[256], p2 = r[320];
    const bool prismatic = model[CH_HDR + m * CH_JNT + 15] != 0.f;
    float g1 = w.n0 * a0 + w.n1 * a1 + w.n2 * a2, g2 = g1;
    if (prismatic) {
        c[0] = a0; c[1] = a1; c[2] = a2;
    } else {
        float d0 = ee[0] - p0, d1 = ee[1] - p1, d2 = ee[2] - p2;
        c[0] = a1 * d2 - a2 * d1;
        c[1] = a2 * d0 - a0 * d2;
        c[2] = a0 * d1 - a1 * d0;
        d0 = w.x0 - p0; d1 = w.x1 - p1; d2 = w.x2 - p2;
        g1 = w.n0 * (a1 * d2 - a2 * d1) + w.n1 * (a2 * d0 - a0 * d2) + w.n2 * (a0 * d1 - a1 * d0);
        d0 = w.y0 - p0; d1 = w.y1 - p1; d2 = w.y2 - p2;
        g2 = w.n0 * (a1 * d2 - a2 * d1) + w.n1 * (a2 * d0 - a0 * d2) + w.n2 * (a0 * d1 - a1 * d0);
    }
    if (m >= n_joints) c[0] = c[1] = c[2] = 0.f;
    return (m < w.f ? g1 : 0.f) - (m < w.f2 ? g2 : 0.f);
}

template <bool REC>
__global__ void __launch_bounds__(64)
chain_ik_clear_kernel(const float* __restrict__ model, const float* __restrict__ targets, const float* __restrict__ obstacles,
                      const float* q_in, int N, int R, int A, const naf_chain_ik_params_t prm, const naf_chain_ik_clear_params_t cp,
                      float* q_out, float* q_work, float* __restrict__ residual_out, float* __restrict__ clear_out,
                      float* __restrict__ iters_out, float* __restrict__ rec_out) {
    extern __shared__ __attribute__((aligned(16))) float ch_lds[];
    const int64_t total = (int64_t)N * R;
    const int64_t cand = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (cand >= total) return;      // (one wave per workgroup and no barrier below)
    const int64_t n = cand / R;
    const int n_joints = (int)model[4], n_seg = (int)model[2], n_pairs = (int)model[9];
    float* ax = ch_lds + threadIdx.x;
    float* ends = ax + (size_t)A * 6 * 64;
    float* q = q_work + cand * A;
    float* keep = q_out + cand * A;
    for (int m = 0; m < A; ++m) {
        const float v = q_in[cand * A + m];
        q[m] = v;
        keep[m] = v;
        if constexpr (REC) iters_out[cand * A + m] = v;
    }
    const float g0 = targets[n * 3], g1 = targets[n * 3 + 1], g2 = targets[n * 3 + 2];
    const float o0 = obstacles[n * 3], o1 = obstacles[n * 3 + 1], o2 = obstacles[n * 3 + 2];
    const int K = prm.iterations;
    float* out4 = clear_out + cand * 4;
    float best_key = -INFINITY;
    for (int k = 0;; ++k) {
        ClearWitness w;
        float ee[3];
        ikc_walk(model, A, n_seg, q, o0, o1, o2, cp.obstacle_radius, ax, ends, ee, w);
        ikc_pairs(model, A, n_seg, n_pairs, ends, w);
        float e0 = g0 - ee[0], e1 = g1 - ee[1], e2 = g2 - ee[2];
        const float len = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
        const float key = len <= cp.tolerance ? fminf(w.c, cp.clearance_goal) : -INFINITY;
        if (k == 0) {      // iterate 0 is the input pose
            best_key = key;
            residual_out[cand] = len;
            out4[0] = w.c; out4[1] = w.c; out4[2] = 0.f; out4[3] = (float)w.kind;
            if (w.c >= cp.clearance_goal || len > cp.tolerance) {      // it keeps the goal, or is not converged: back bit for bit
                if constexpr (REC) {
                    for (int u = 0; u < K; ++u) {
                        float* it = iters_out + ((int64_t)(u + 1) * total + cand) * A;
                        float* rc = rec_out + ((int64_t)u * total + cand) * (A + 2);
                        for (int m = 0; m < A; ++m) { it[m] = keep[m]; rc[m] = 0.f; }
                        rc[A] = w.c; rc[A + 1] = (float)w.kind;
                    }
                }
                return;
            }
        } else if (key > best_key) {      // (ties stay with the earliest)
            best_key = key;
            for (int m = 0; m < A; ++m) keep[m] = q[m];
            residual_out[cand] = len;
            out4[1] = w.c; out4[2] = (float)k; out4[3] = (float)w.kind;
        }
        if (k == K) break;
        if (len > prm.e_max) {
            const float s = prm.e_max / len;
            e0 *= s; e1 *= s; e2 *= s;
        }
        // pass 1 over LDS: M = sum c c^T + lam^2 I and the second right-hand side b = sum c gamma
        float m00 = prm.lam2, m01 = 0.f, m02 = 0.f, m11 = prm.lam2, m12 = 0.f, m22 = prm.lam2, b0 = 0.f, b1 = 0.f, b2 = 0.f;
        for (int m = 0; m < A; ++m) {
            float c[3];
            const float gamma = ikc_column(model, m, n_joints, ax, ee, w, c);
            m00 += c[0] * c[0]; m01 += c[0] * c[1]; m02 += c[0] * c[2];
            m11 += c[1] * c[1]; m12 += c[1] * c[2]; m22 += c[2] * c[2];
            b0 += c[0] * gamma; b1 += c[1] * gamma; b2 += c[2] * gamma;
        }
        const float c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
        const float c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const float det = m00 * c00 + m01 * c01 + m02 * c02;
        const float y0 = (c00 * e0 + c01 * e1 + c02 * e2) / det, y1 = (c01 * e0 + c11 * e1 + c12 * e2) / det,
                    y2 = (c02 * e0 + c12 * e1 + c22 * e2) / det;
        const float z0 = (c00 * b0 + c01 * b1 + c02 * b2) / det, z1 = (c01 * b0 + c11 * b1 + c12 * b2) / det,
                    z2 = (c02 * b0 + c12 * b1 + c22 * b2) / det;
        // pass 2: dq_m = c_m . y and h_m = gamma_m - c_m . z into the record's first two floats; max |dq_m|, max |h_m|, sigma
        float big = 0.f, top = 0.f, sigma = 0.f;
        float* rc = REC ? rec_out + ((int64_t)k * total + cand) * (A + 2) : nullptr;
        for (int m = 0; m < A; ++m) {
            float c[3];
            const float gamma = ikc_column(model, m, n_joints, ax, ee, w, c);
            const float dq = c[0] * y0 + c[1] * y1 + c[2] * y2;
            const float h = gamma - (c[0] * z0 + c[1] * z1 + c[2] * z2);
            ax[m * 6 * 64] = dq;
            ax[m * 6 * 64 + 64] = h;
            big = fmaxf(big, fabsf(dq));
            top = fmaxf(top, fabsf(h));
            sigma += gamma * h;
            if constexpr (REC) rc[m] = gamma;
        }
        if constexpr (REC) { rc[A] = w.c; rc[A + 1] = (float)w.kind; }
        const float scale = big > prm.dq_max ? prm.dq_max / big : 1.f;
        float coef = 0.f;
        if (k < K - cp.settle && w.c < cp.clearance_goal && sigma > IKC_SIGMA_FLOOR) {
            coef = (cp.clearance_goal - w.c) / sigma;      // the Gauss-Newton length that lifts the one active test to the goal
            const float far = fabsf(coef) * top;
            if (far > cp.push_max) coef *= cp.push_max / far;
        }
        float* it = REC ? iters_out + ((int64_t)(k + 1) * total + cand) * A : nullptr;
        for (int m = 0; m < A; ++m) {
            const float* j = model + CH_HDR + m * CH_JNT;
            float v = q[m] + scale * ax[m * 6 * 64] + coef * ax[m * 6 * 64 + 64];
            if (j[16] != 0.f) {
                if (v > j[18]) v = j[18];
                if (v < j[17]) v = j[17];
            }
            q[m] = v;
            if constexpr (REC) it[m] = v;
        }
    }
}

extern "C" int naf_chain_ik_clear(naf_chain_env_t* h, const float* targets_dev, const float* obstacles_dev, const float* q_in_dev, int N,
                                  int R, naf_chain_ik_params_t params, naf_chain_ik_clear_params_t clear_params, float* q_out,
                                  float* q_work, float* residual_out, float* clear_out, float* iters_out, float* rec_out,
                                  void* stream) {
    if (!h || !targets_dev || !obstacles_dev || !q_in_dev || !q_out || !q_work || !residual_out || !clear_out ||
        !ch_ik_counts_ok(N, R) || (iters_out == nullptr) != (rec_out == nullptr) || q_work == q_out || q_work == q_in_dev)
        return NAF_ERR_ARG;
    if (params.iterations < 1 || params.iterations > 1 << 20 || !std::isfinite(params.lam2) || !(params.lam2 > 0.f) ||
        !std::isfinite(params.e_max) || !(params.e_max > 0.f) || !std::isfinite(params.dq_max) || !(params.dq_max > 0.f))
        return NAF_ERR_ARG;
    if (clear_params.settle < 0 || clear_params.settle > params.iterations || !std::isfinite(clear_params.tolerance) ||
        !(clear_params.tolerance >= 0.f) || !std::isfinite(clear_params.clearance_goal) || !std::isfinite(clear_params.push_max) ||
        !(clear_params.push_max > 0.f) || !std::isfinite(clear_params.obstacle_radius) || !(clear_params.obstacle_radius >= 0.f))
        return NAF_ERR_ARG;
    // 1536 bytes per driven joint and per segment: above what the handle's kernels may ask for there is no launch
    const size_t lds = (size_t)(h->A + h->n_seg) * 6 * 64 * sizeof(float);
    if (lds > CH_MAX_DYN_LDS) return NAF_CHAIN_ERR_LDS;
    int rc = ch_raise<chain_ik_clear_kernel<false>>();
    if (rc == NAF_OK) rc = ch_raise<chain_ik_clear_kernel<true>>();
    if (rc != NAF_OK) return rc;
    const unsigned grid = (unsigned)(((int64_t)N * R + 63) / 64);
    if (iters_out)
        chain_ik_clear_kernel<true><<<grid, 64, lds, (hipStream_t)stream>>>(h->model_dev, targets_dev, obstacles_dev, q_in_dev, N, R, h->A,
                                                                           params, clear_params, q_out, q_work, residual_out, clear_out,
                                                                           iters_out, rec_out);
    else
        chain_ik_clear_kernel<false><<<grid, 64, lds, (hipStream_t)stream>>>(h->model_dev, targets_dev, obstacles_dev, q_in_dev, N, R, h->A,
                                                                            params, clear_params, q_out, q_work, residual_out, clear_out,
                                                                            nullptr, nullptr);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}
