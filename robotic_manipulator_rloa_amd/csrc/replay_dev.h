// The replay ring's handle and its device-side counters, shared by csrc/replay.hip and csrc/step_path.hip.
#pragma once
#include "common.h"
#include "../../include/naf_hip.h"

struct naf_replay {
    uint64_t capacity;
    int S, A, row_floats;
    float* rows;
    uint64_t* meta;  // {head, size, total_added, sample_counter, -, -, -, bad_index_count}
    uint32_t magic;
};
#define NAF_REPLAY_MAGIC 0x4e414652u

enum { META_HEAD = 0, META_SIZE = 1, META_TOTAL = 2, META_SAMPLE_CTR = 3, META_BAD_IDX = 7 };

#ifdef __HIPCC__
// the leading floats of a ring row as the learner sees them: `.long()` of the reference on the action columns [lo, hi); f0 = the
// column of v.x (the gathers of csrc/step_path.hip and csrc/vector_step.hip)
__device__ __forceinline__ static float4 naf_row_trunc4(float4 v, int f0, int lo, int hi) {
    if (f0 + 3 >= lo && f0 < hi) {
        if (f0 + 0 >= lo && f0 + 0 < hi) v.x = truncf(v.x);
        if (f0 + 1 >= lo && f0 + 1 < hi) v.y = truncf(v.y);
        if (f0 + 2 >= lo && f0 + 2 < hi) v.z = truncf(v.z);
        if (f0 + 3 >= lo && f0 + 3 < hi) v.w = truncf(v.w);
    }
    return v;
}
#endif

