// ca_trace.h -- the small kernels of a recording rollout (ca_rollout_trace / ca_alan_rollout_trace)
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
//
// A record is the state after a whole number of steps: the selected planes of pos_x, pos_y, vel_x, vel_y ([A*N] each) and the
// arena's three words step_count, arena_done, episode ([A] each), as ca_get would read them there.  Two ways lead into the caller's
// buffers:
//   * a rollout that is a sequence of launches per step (the one-lane kernels, the two-lanes kernel, the tiled path, the three-launch
//     ALAN step, anything with an observation): trace_record_kernel below, enqueued behind the launches of a step whose number is a
//     multiple of `every` -- the stream orders it behind the stores it copies;
//   * a rollout that is one launch per 256 steps: the Trace instantiations of the four-lanes kernel store from their registers
//     (ca_quad.h); trace_setup_kernel writes their cursor into the handle's TraceDev block in front of every such launch.
#pragma once
#include "ca_common.h"

namespace ca {

// one record: src = the handle's planes in the record's order, words = step_count | arena_done | episode; agents / arenas point at
// the record itself (the host has added r * C * an and r * 3 * A)
struct TraceRecArgs {
    const float* src[4];
    const int* words[3];
    float* agents;
    int* arenas;   // or null
    unsigned an;   // A * N
    int A, C;
};

// one lane per agent, agent fastest: C coalesced copies of 4 B per lane; the first A lanes copy the arena's words as well
__global__ __launch_bounds__(256) void trace_record_kernel(const TraceRecArgs t) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g < t.an) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < t.C) t.agents[(size_t)c * t.an + g] = t.src[c][g];
    }
    if (t.arenas != nullptr && g < (unsigned)t.A) {
#pragma unroll
        for (int w = 0; w < 3; ++w) t.arenas[(size_t)w * t.A + g] = t.words[w][g];
    }
}

// the trace block of the next Trace launch of the four-lanes kernel, by value through the kernel arguments: ordered on the stream
// like the launch that reads it, and no host memory has to outlive the call
__global__ void trace_setup_kernel(TraceDev* dst, const TraceDev v) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst = v;
}

}  // namespace ca
